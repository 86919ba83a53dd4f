"""CPU proof of forward_ref.py's bounds: honest emulations of each kernel's arithmetic stay inside their bound at every element, for every case the GPU test
(test_forward_fp64_gpu.py) runs, and subtly wrong arithmetic falls outside.  No bound goes to the GPU unproven.

Emulations (torch on the CPU, fp32 where the kernels are fp32; the summation ORDER inside a chunk is torch's, not the kernels' — the bounds are order-free):
  * RoPE in the storage dtype's own arithmetic (torch rounds every elementwise op of a 16-bit tensor): must equal the float64 chain bit for bit;
  * RMSNorm / LayerNorm with fp32 statistics and the kernels' rounding points;
  * the fp32-P decode family: fp32 scores in the log2 domain, chunks of the kernel's size reduced to {o, max, sum}, merged in chunk order, the newest key folded
    in last (decode_attn_step / decode_fused), or no newest key (decode_attn), or 64-key pieces (the batch's wave kernel);
  * the MFMA prefill: P rounded to T, fp32 accumulation over 64-key tiles with the online rescale, lse = m + log2 l.

Worst err / bound of the honest emulations over all cases (printed by the tests, `pytest -s`).  For a 16-bit output the ratio is quantised — a result one
ulp_T from round_T(ref) scores 1 ulp / (1 ulp + E), just under 1, and that is what the 16-bit columns of the fp32-P family and LayerNorm show; the float column
measures the derived fp32 term itself:
    RoPE                 float 0.65                16-bit: equality
    RMSNorm              float 0.25                16-bit: equality outside the flippable set (0.1 % of f16 elements differ inside it), largest flippable share
                                                   of a row 0.0098
    LayerNorm            float 0.14                bf16 / f16 0.999 / 0.997
    decode_attn          float 0.056 (0.47 on the crafted two-key input)       bf16 / f16 0.99 / 0.98
    decode step / fused  float 0.135, appended key 0.54                        bf16 / f16 0.59 / 0.99
    batch wave form      float 0.084                                            bf16 / f16 0.01 / 0.99
    prefill              output bf16 / f16 0.66 / 0.67, the fp32 part at most 0.06 / 0.97 of u_T mag (the forced-rescale input in f16), lse 0.06
The fp32-P bounds are worst-case (every rounding counted at full size and with one sign), hence ratios near 0.1 rather than 0.5 on long sums.
Mutants (each must violate its bound): the newest key dropped; one cached key with p < 1e-3 dropped; the last key of a 128-key chunk dropped (flat input: with
randn keys that key's weight can be 1e-5 and nothing could see it); log2(e) taken as 1.4427 (a crafted float input: two keys 6 log2 units apart, the heavy one
with a zero value row — on randn inputs the constant's 3.4e-6 hides under the worst-case score bound); the causal mask admitting one future key for rows >= 64;
one chunk's merge weight from the wrong maximum; P rounded to 16 bits where fp32 is kept; RoPE as one fma; RMSNorm with a single final rounding; LayerNorm with
one-pass variance on the offset row (float: in bf16 that row IS constant, 100 + 0.01 randn rounds to 100, and x - mean is exactly 0 whatever rstd is; in f16 a
few elements stand 1/16 off 100 and both row sums are exact in fp32 up to H = 1677 — E[x^2] - mean^2 is then honest arithmetic, not a mutant)."""
import math

import pytest
import torch

import forward_ref as F
from forward_ref import DT


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ---- emulations ---------------------------------------------------------------------------------------------------------------------------------------------------
def emu_rope(x, pos, table, dt):
    """T( T(x c) + T(rot s) ) in T's own arithmetic."""
    D = x.shape[-1]
    tb = table.to(DT[dt])
    c = torch.cat([tb[pos, : D // 2]] * 2, -1)[:, None, :]
    s = torch.cat([tb[pos, D // 2:]] * 2, -1)[:, None, :]
    rot = torch.cat([-x[..., D // 2:], x[..., : D // 2]], -1)
    return (x * c) + (rot * s)


def mutant_rope_fma(x, pos, table, dt):
    """The product rounding skipped: T( x c + T(rot s) ), one fma."""
    D = x.shape[-1]
    tb = table.to(DT[dt]).double()
    c = torch.cat([tb[pos, : D // 2]] * 2, -1)[:, None, :]
    s = torch.cat([tb[pos, D // 2:]] * 2, -1)[:, None, :]
    xd = x.double()
    rot = torch.cat([-xd[..., D // 2:], xd[..., : D // 2]], -1)
    return (xd * c + F.rnd(rot * s, dt)).to(DT[dt])


def emu_rmsnorm(x, w, dt, eps, single_rounding=False):
    x32 = x.float()
    inv = torch.rsqrt((x32 * x32).sum(-1, keepdim=True) / x.shape[-1] + _f32(eps))
    if single_rounding:
        return (x32 * inv * w.float()).to(DT[dt])
    return ((x32 * inv).to(DT[dt]).float() * w.float()).to(DT[dt])


def emu_layernorm(x, w, b, dt, eps, one_pass=False):
    x32 = x.float()
    H = x.shape[-1]
    mean = x32.sum(-1, keepdim=True) / H
    if one_pass:
        var = ((x32 * x32).sum(-1, keepdim=True) / H - mean * mean).clamp_min(0)
    else:
        d = x32 - mean
        var = (d * d).sum(-1, keepdim=True) / H
    rstd = torch.rsqrt(var + _f32(eps))
    return ((x32 - mean) * rstd * w.float() + b.float()).to(DT[dt])


def emu_fp32_row(q, k, v, dt, chunk, newest_last, drop=None, log2e=F.LOG2E, wrong_max=False, p16=False, drop_newest=False):
    """One query row q [nh, D] over keys k / v [n, nkv, D]: the fp32-P family.  Mutants: drop = a key index that is skipped, log2e, wrong_max (chunk 0 weighted with
    the last chunk's maximum), p16 (P rounded to 16 bits), drop_newest."""
    nh, D = q.shape
    n, nkv, _ = k.shape
    rep = nh // nkv
    q32 = q.float(); k32 = k.float().repeat_interleave(rep, 1); v32 = v.float().repeat_interleave(rep, 1)
    scl = _f32(1.0 / math.sqrt(D)) * _f32(log2e)
    s = torch.einsum("hd,khd->hk", q32, k32) * scl
    n_c = n - 1 if newest_last else n
    keep = torch.ones(n, dtype=torch.bool)
    if drop is not None:
        keep[drop] = False
    parts = []
    for c0 in range(0, n_c, chunk):
        sel = torch.arange(c0, min(c0 + chunk, n_c))[keep[c0:min(c0 + chunk, n_c)]]
        if sel.numel() == 0:
            continue
        sc = s[:, sel]
        m = sc.max(-1).values
        e = torch.exp2(sc - m[:, None])
        l = e.sum(-1)
        if p16:
            e = e.to(DT[dt] if dt != "f32" else torch.float16).float()
        parts.append((m, l, torch.einsum("hk,khd->hd", e, v32[sel])))
    l = torch.zeros(nh); o = torch.zeros(nh, D); M = torch.full((nh,), float("-inf"))
    if parts:
        M = torch.stack([p[0] for p in parts]).max(0).values
        for i, (m, lc, oc) in enumerate(parts):
            w = torch.exp2((parts[-1][0] if wrong_max and i == 0 else m) - M)
            l = l + w * lc
            o = o + w[:, None] * oc
    if newest_last and not drop_newest:
        s_new = s[:, n - 1]
        M2 = torch.maximum(M, s_new)
        wa = torch.exp2(M - M2); wb = torch.exp2(s_new - M2)
        o = wb[:, None] * v32[n - 1] + wa[:, None] * o
        l = wa * l + wb
    return (o / l[:, None]).to(DT[dt])


def emu_decode_attn(q, k, v, dt, past, causal, n_split, **mut):
    """decode_attn_kernel: row r sees past + r + 1 keys (causal) or all; a split holds ceil(ceil(n / n_split) / 64) 64 keys."""
    out = []
    for r in range(q.shape[0]):
        n = past + r + 1 if causal else k.shape[0]
        chunk = (((n + n_split - 1) // n_split + 63) // 64) * 64
        out.append(emu_fp32_row(q[r], k[:n], v[:n], dt, chunk, False, **mut))
    return torch.stack(out)


def emu_prefill(q, k, v, dt, causal, past, future_key=False):
    """flash_prefill2_kernel's arithmetic: 64-key tiles, fp32 scores in the log2 domain, online max / rescale, P rounded to T for P V, l from the unrounded P.
    Returns (out [Tq, nh, D] in T, lse [nh, Tq] fp32).  future_key: the causal mask admits key pos + 1 for rows >= 64."""
    Tq, nh, D = q.shape
    Tk, nkv, _ = k.shape
    rep = nh // nkv
    q32 = q.float().permute(1, 0, 2); k32 = k.float().repeat_interleave(rep, 1).permute(1, 0, 2); v32 = v.float().repeat_interleave(rep, 1).permute(1, 0, 2)
    scl = _f32(1.0 / math.sqrt(D)) * _f32(F.LOG2E)
    m = torch.full((nh, Tq), -1e30); l = torch.zeros(nh, Tq); O = torch.zeros(nh, Tq, D)
    rows = torch.arange(Tq)
    lim = past + rows + (rows >= 64).long() * int(future_key) if causal else torch.full((Tq,), Tk)
    for t0 in range(0, Tk, 64):
        S = (q32 @ k32[:, t0:t0 + 64].transpose(1, 2)) * scl
        vis = torch.arange(t0, min(t0 + 64, Tk))[None, :] <= lim[:, None]
        S = S.masked_fill(~vis[None], float("-inf"))
        m_new = torch.maximum(m, S.max(-1).values)
        alpha = torch.exp2(m - m_new)
        e = torch.exp2(S - m_new[..., None])
        l = l * alpha + e.sum(-1)
        O = O * alpha[..., None] + e.to(DT[dt]).float() @ v32[:, t0:t0 + 64]
        m = m_new
    return (O / l[..., None]).permute(1, 0, 2).to(DT[dt]), m + torch.log2(l)


WORST = {}


def _note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"worst err / bound, {family}: {ratio:.3f} (so far {WORST[family]:.3f})")


# ---- RoPE ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.ROPE_DTYPES)
@pytest.mark.parametrize("D,nh,nkv", F.ROPE_GEOMS)
def test_rope_chain(dt, D, nh, nkv):
    table = F.rope_table(F.ROPE_S_MAX, D)
    differs = 0
    for T in F.ROPE_T:
        x = F.rope_inputs(D, nh, nkv, T, dt)[:, : (nh + nkv) * D].reshape(T, nh + nkv, D)
        for pos0 in F.rope_pos0(T):
            pos = torch.arange(pos0, pos0 + T)
            _note("rope " + dt, F.rope_check(emu_rope(x, pos, table, dt), x, pos, table, dt, f"T {T} pos0 {pos0}"))
            if dt == "f16":
                bad = mutant_rope_fma(x, pos, table, dt)
                n = int((bad.double() != F.rope_chain(x, pos, table, dt)[0]).sum())
                differs += n
                if n:
                    with pytest.raises(AssertionError):
                        F.rope_check(bad, x, pos, table, dt)
    if dt == "f16":
        assert differs > 0, "the one-fma mutant must differ from the chain somewhere on the test's own inputs"
        print(f"one-fma mutant: {differs} f16 elements differ")


def test_rope_mutants_sign_and_index():
    """A wrong sign in one half and a cos / sin row that is off by one are caught by equality as a matter of course."""
    D, T, dt = 64, 65, "bf16"
    table = F.rope_table(F.ROPE_S_MAX, D)
    x = F.rope_inputs(D, 4, 2, T, dt)[:, : 4 * D].reshape(T, 4, D)
    pos = torch.arange(37, 37 + T)
    good = emu_rope(x, pos, table, dt)
    flipped = good.clone(); flipped[..., D // 2:] = emu_rope(x, pos, -table, dt)[..., D // 2:]
    for bad in (flipped, emu_rope(x, pos + 1, table, dt)):
        with pytest.raises(AssertionError):
            F.rope_check(bad, x, pos, table, dt)


# ---- norms --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("H", F.RMS_H)
def test_rmsnorm(dt, H):
    for rows in F.NORM_ROWS:
        x, w, _ = F.norm_inputs(rows, H, dt)
        r, frac = F.rmsnorm_check(emu_rmsnorm(x, w, dt, F.NORM_EPS), x, w, dt, what=f"{rows} x {H}")
        _note("rmsnorm " + dt, r)
        _note("rmsnorm flippable share " + dt, frac)
        if dt != "f32" and rows == 70:                              # for float there is no intermediate rounding to skip; 3 rows of 8 can agree by chance
            with pytest.raises(AssertionError):
                F.rmsnorm_check(emu_rmsnorm(x, w, dt, F.NORM_EPS, single_rounding=True), x, w, dt)


@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("H", F.LN_H)
def test_layernorm(dt, H):
    for rows in F.NORM_ROWS:
        x, w, b = F.norm_inputs(rows, H, dt)
        _note("layernorm " + dt, F.layernorm_check(emu_layernorm(x, w, b, dt, F.NORM_EPS), x, w, b, dt, what=f"{rows} x {H}"))
        if dt == "f32":                                             # 16-bit: the offset row is (all but) constant and its sums are exact in fp32, see above
            off = slice(rows, rows + 1)
            with pytest.raises(AssertionError):
                F.layernorm_check(emu_layernorm(x[off], w, b, dt, F.NORM_EPS, one_pass=True), x[off], w, b, dt)


# ---- prefill ------------------------------------------------------------------------------------------------------------------------------------------------------
def _prefill_case(dt, q, k, v, causal, past, what):
    R = F.AttnRef(q, k, v, causal, past)
    got, lse = emu_prefill(q, k, v, dt, causal, past)
    _note("prefill " + dt, F.check(got, R.ref, R.prefill_bound(dt), dt, what))
    _note("prefill lse", F.check(lse, R.lse2, R.lse_bound(), "f32", what + " lse"))
    part = float((R.prefill_fp32_part(dt) / (F.UT[dt] * R.mag)).max())
    _note("prefill fp32 part / (u_T mag) " + dt, part)
    assert part <= 1.0, f"{what}: the fp32 arithmetic does not fit the second u_T mag for this input ({part:.2f})"
    return R


@pytest.mark.parametrize("dt", F.PREFILL_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("D,nh,nkv,Tq,past,causal", F.PREFILL_CASES)
def test_prefill(dt, flat, D, nh, nkv, Tq, past, causal):
    q, k, v = F.attn_inputs(D, nh, nkv, Tq, past + Tq, dt, Tq + D, flat)
    R = _prefill_case(dt, q, k, v, causal, past, f"prefill {D} {nh} {nkv} {Tq} {past} {causal} flat {flat}")
    if causal and Tq > 65:
        with pytest.raises(AssertionError):
            F.check(emu_prefill(q, k, v, dt, causal, past, future_key=True)[0], R.ref, R.prefill_bound(dt), dt)


@pytest.mark.parametrize("dt", F.PREFILL_DTYPES)
def test_prefill_forced_rescale(dt):
    q, k, v = F.forced_rescale_inputs(dt)
    _prefill_case(dt, q, k, v, True, 0, "forced rescale")


# ---- the fp32-P decode family -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("D,nh,nkv,rows,past,causal,n_split", F.DECODE_CASES)
def test_decode_attn(dt, flat, D, nh, nkv, rows, past, causal, n_split):
    Tk = past + rows if causal else F.DECODE_NONCAUSAL_KEYS
    q, k, v = F.attn_inputs(D, nh, nkv, rows, Tk, dt, rows + past, flat)
    R = F.AttnRef(q, k, v, causal, past)
    E = R.decode_attn_bound(n_split)
    _note("decode_attn " + dt, F.check(emu_decode_attn(q, k, v, dt, past, causal, n_split), R.ref, E, dt, "decode_attn"))
    if past >= 700:
        muts = [dict(wrong_max=True), dict(p16=True)]
        if flat:
            muts.append(dict(drop=191))                               # the last key of the first split: 192 keys at 1101 / 8 and at 701 / 4
        for mut in muts:
            with pytest.raises(AssertionError):
                F.check(emu_decode_attn(q, k, v, dt, past, causal, n_split, **mut), R.ref, E, dt)


@pytest.mark.parametrize("dt", F.DECODE_DTYPES)
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("nh,nkv,D", F.STEP_GEOMS)
@pytest.mark.parametrize("pos", F.STEP_POS)
def test_decode_step(dt, flat, nh, nkv, D, pos):
    """decode_attn_step / decode_fused (128-key chunks, newest key folded last) and the batch's wave form (64-key pieces) on the same step."""
    table = F.rope_table(F.STEP_S_MAX, D)
    row, k_past, v_past = F.step_inputs(nh, nkv, D, pos, dt, flat=flat)
    R, k_new, kE, v_new = F.step_ref(row, k_past, v_past, table, pos, nh, nkv, D, dt)
    p1 = torch.tensor([pos])
    q_e = emu_rope(row[: nh * D].view(1, nh, D), p1, table, dt)
    k_e = emu_rope(row[nh * D:(nh + nkv) * D].view(1, nkv, D), p1, table, dt)
    _note("append " + dt, F.append_check(k_e[0], k_new, kE, dt, "appended key"))
    k_all = torch.cat([k_past, k_e], 0); v_all = torch.cat([v_past, v_new[None]], 0)
    E = R.step_bound(pos // 128 + 1)
    got = emu_fp32_row(q_e[0], k_all, v_all, dt, 128, True)
    _note("decode step " + dt, F.check(got[None], R.ref, E, dt, f"step pos {pos}"))
    _note("batch wave " + dt, F.check(emu_fp32_row(q_e[0], k_all, v_all, dt, 64, True)[None], R.ref, R.batch_wave_bound(), dt, f"wave pos {pos}"))
    if pos == 300:
        muts = [dict(drop_newest=True), dict(wrong_max=True), dict(p16=True)]
        if flat:
            muts.append(dict(drop=127))                               # the last key of a 128-key chunk, p = 1 / 301
        for mut in muts:
            with pytest.raises(AssertionError):
                F.check(emu_fp32_row(q_e[0], k_all, v_all, dt, 128, True, **mut)[None], R.ref, E, dt)
        if not flat:                                                  # head 0 alone loses the heaviest of its cached keys with p < 1e-3
            p0 = R.P[0, 0, :pos]
            small = torch.where(p0 < 1e-3, p0, torch.zeros_like(p0))
            assert 0 < float(small.max()) < 1e-3
            bad = got.clone()
            bad[0] = emu_fp32_row(q_e[0], k_all, v_all, dt, 128, True, drop=int(small.argmax()))[0]
            with pytest.raises(AssertionError):
                F.check(bad[None], R.ref, E, dt)


def test_truncated_log2e_is_caught():
    """log2(e) taken as 1.4427 scales every score by 1 + 3.4e-6: only score DIFFERENCES between keys that both carry weight see it.  Two keys, 6 log2 units apart,
    no cancellation inside the dot products (A = |s|), the heavy key's value row zero (mag is the light key's 1 / 65): the weight ratio is off by
    ln 2 x 3.4e-6 x 6 = 1.4e-5 = 237 U against a bound of a few dozen U.  The honest emulation passes the same input."""
    D, dt = 64, "f32"
    q = torch.full((1, 1, D), 0.5)
    s_target = 6.0 / F.LOG2E * math.sqrt(D)                            # q . k for 6 log2 units
    k = torch.stack([torch.zeros(1, D), torch.full((1, D), s_target / (0.5 * D))])
    v = torch.stack([torch.randn(1, D, generator=F.gen(5)), torch.zeros(1, D)])
    R = F.AttnRef(q, k, v, False, 0)
    E = R.decode_attn_bound(1)
    _note("decode_attn f32 (crafted)", F.check(emu_decode_attn(q, k, v, dt, 0, False, 1), R.ref, E, dt, "honest"))
    with pytest.raises(AssertionError):
        F.check(emu_decode_attn(q, k, v, dt, 0, False, 1, log2e=1.4427), R.ref, E, dt)
