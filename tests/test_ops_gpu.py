"""Per-kernel parity: every HIP kernel on the path vs a plain torch fp32 statement of the same op (the reference's
arithmetic lives in torch/transformers, so torch fp32 on the same inputs is the op-level oracle).  All calls go
through the C ABI (`lmx_op_*`)."""
import math

import pytest
import torch

import forward_ref as FR
import linear_ref as L

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# relative-to-magnitude tolerances per storage dtype (fp32 accumulate everywhere).  The linears are ALSO held, element by element, to the float64 statements of
# linear_ref.py: one ulp of the once-rounded float64 result for the 16-bit GEMMs, ulp_T(ref) + the derived fp32 bound for the fp32 GEMM and the GEMV family.
TOL = {"bf16": 1.2e-2, "f16": 2e-3, "f32": 2e-5}


def _gemm_check(got, x, w, dt, what, bias=None, residual=None, act=0):
    """Per-element check of one GEMM output (w: the [N, K] weight, or the (gate, up) pair for SiLU*mul)."""
    if dt == "f32":                                             # gemm_f32_kernel: one fmaf chain of K terms per output, no tree
        ref, E, _ = L.linear_ref(x, w, dt, bias=bias, residual=residual, act=act, chain=x.shape[1], tree=0)
        L.check(got, ref, E, dt, what)
        return
    if act == L.ACT_SILU_MUL:
        ref = L.act64(x.double() @ w[0].double().t(), act)[0] * (x.double() @ w[1].double().t())
    else:
        y = x.double() @ w.double().t()
        ref = L.act64(y + bias.double() if bias is not None else y, act)[0]
        ref = ref + residual.double() if residual is not None else ref
    L.gemm16_check(got, ref, dt, act != 0, what)


def _rel_err(got, ref):
    got = got.float().cpu(); ref = ref.float().cpu()
    return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def _act_ref(y, act):
    from llava_mi355x import _C
    if act == _C.ACT_QUICK_GELU:
        return y * torch.sigmoid(1.702 * y)
    if act == _C.ACT_GELU_ERF:
        return torch.nn.functional.gelu(y)
    return y


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("variant", [0, 2, 4, 5, 7, 9, 15, 16, 17, 18])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (1087, 512, 256), (577, 384, 640), (33, 136, 128), (300, 1024, 1024)])
def test_gemm_plain(cuda, dt, variant, M, N, K):
    from llava_mi355x import ops
    if dt == "f32" and variant != 0:
        pytest.skip("fp32 verification GEMM has one variant")
    torch.manual_seed(M * 7 + N)
    x = torch.randn(M, K, device=cuda).to(DT[dt]); w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(DT[dt])
    got = ops.gemm(x, w, variant=variant)
    ref = x.float() @ w.float().t()
    assert _rel_err(got, ref) < TOL[dt]
    _gemm_check(got, x, w, dt, f"variant {variant} {M}x{N}x{K} {dt}")


def test_gemm_is_transpose_detecting(cuda):
    """A = identity-like probe with asymmetric W: catches row/col swaps in the MFMA C/D mapping."""
    from llava_mi355x import ops
    M = N = 128; K = 128
    x = torch.eye(M, K, device=cuda, dtype=torch.bfloat16)
    w = (torch.arange(N, device=cuda).float()[:, None] * 0.25 + torch.arange(K, device=cuda).float()[None, :] * 0.001953125).to(torch.bfloat16)
    for variant in (0, 2, 4, 5, 7, 9, 15, 16, 17, 18):
        got = ops.gemm(x, w, variant=variant)
        assert torch.equal(got.float().cpu(), (x.float() @ w.float().t()).to(torch.bfloat16).float().cpu())


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_gemm_bias_act_residual(cuda, dt, act):
    from llava_mi355x import ops
    torch.manual_seed(act)
    M, N, K = 577, 256, 192
    x = torch.randn(M, K, device=cuda).to(DT[dt]); w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(DT[dt])
    b = torch.randn(N, device=cuda).to(DT[dt]); r = torch.randn(M, N, device=cuda).to(DT[dt])
    got = ops.gemm(x, w, bias=b, residual=r, act=act)
    ref = _act_ref(x.float() @ w.float().t() + b.float(), act) + r.float()
    assert _rel_err(got, ref) < TOL[dt]
    _gemm_check(got, x, w, dt, f"act {act} {dt}", bias=b, residual=r, act=act)
    # in-place residual (C aliases R), the way the engine keeps the residual stream
    r2 = r.clone()
    ops.gemm(x, w, bias=b, residual=r2, act=act, out=r2)
    assert _rel_err(r2, ref) < TOL[dt]
    assert torch.equal(r2, got)


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("M", [1, 77, 1087])
def test_gemm_silu_mul(cuda, dt, M):
    from llava_mi355x import _C, ops
    torch.manual_seed(5)
    I, K = 352, 256
    x = torch.randn(M, K, device=cuda).to(DT[dt])
    g = (torch.randn(I, K, device=cuda) / math.sqrt(K)).to(DT[dt]); u = (torch.randn(I, K, device=cuda) / math.sqrt(K)).to(DT[dt])
    fused = ops.interleave_gate_up(g, u)
    ref = torch.nn.functional.silu(x.float() @ g.float().t()) * (x.float() @ u.float().t())
    for variant in ((0,) if dt == "f32" else (0, 2, 4, 7, 9, 18)):
        got = ops.gemm(x, fused, act=_C.ACT_SILU_MUL, variant=variant)
        assert got.shape == (M, I)
        assert _rel_err(got, ref) < TOL[dt], f"variant {variant}"
        _gemm_check(got, x, (g, u), dt, f"SiLU*mul variant {variant} M={M} {dt}", act=_C.ACT_SILU_MUL)
    if M <= 4:
        got2 = ops.gemv(x, fused, act=_C.ACT_SILU_MUL)
        assert _rel_err(got2, ref) < TOL[dt]
        L.check(got2, *L.linear_ref(x, (g, u), dt, act=_C.ACT_SILU_MUL)[:2], dt, f"gemv SiLU*mul {dt}")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("MB,N,K", [(1, 4096, 4096), (1, 1000, 11008), (3, 264, 512), (4, 4096, 1024)])
def test_gemv(cuda, dt, MB, N, K):
    from llava_mi355x import ops
    torch.manual_seed(N + MB)
    x = torch.randn(MB, K, device=cuda).to(DT[dt]); w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(DT[dt])
    b = torch.randn(N, device=cuda).to(DT[dt]); r = torch.randn(MB, N, device=cuda).to(DT[dt])
    got = ops.gemv(x, w, bias=b, residual=r)
    ref = x.float() @ w.float().t() + b.float() + r.float()
    assert _rel_err(got, ref) < TOL[dt]
    L.check(got, *L.linear_ref(x, w, dt, bias=b, residual=r)[:2], dt, f"gemv bias + residual {dt}")
    # fused RMSNorm prologue
    g = (1 + 0.1 * torch.randn(K, device=cuda)).to(DT[dt])
    got = ops.gemv(x, w, norm_w=g, eps=1e-5)
    xf = x.float()
    xn = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(DT[dt]).float() * g.float()
    ref = xn.to(DT[dt]).float() @ w.float().t()
    assert _rel_err(got, ref) < TOL[dt]
    _gemv_norm_check(got, x, w, dt, g, f"gemv norm {dt}")


def _gemv_norm_check(got, x, w, dt, g, what, act=0):
    """Per-element check of a GEMV with the RMSNorm prologue; the flippable set of these (device-drawn) inputs must stay under linear_ref's cap."""
    ref, E, frac = L.linear_ref(x, w, dt, norm_w=g, eps=1e-5, act=act)
    assert frac <= L.FLIP_MAX_FRACTION, f"{what}: flippable fraction {frac:.4f}"
    L.check(got, ref, E, dt, what)


# the decode linears of LLaVA-1.5-7B / 13B at their REAL shapes, each with the epilogue / prologue the decode step fuses into it:
# q|k|v = RMSNorm prologue, o_proj / down_proj = residual add, gate|up = RMSNorm prologue + SiLU*mul epilogue.  gemv2_kernel is what lmx_op_gemv runs for one
# 16-bit row; the reference is torch fp32 with HF's rounding point (the normalised row rounded to the model dtype before the product).
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("H,I,nh", [(4096, 11008, 32), (5120, 13824, 40)])
def test_gemv2_real_decode_shapes(cuda, dt, H, I, nh):
    from llava_mi355x import _C, ops
    torch.manual_seed(H)
    T = DT[dt]
    def W(n, k): return (torch.randn(n, k, device=cuda) / math.sqrt(k)).to(T)
    def rms(x, g, eps=1e-5):
        xf = x.float()
        return ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)).to(T).float() * g.float()).to(T).float()
    h = torch.randn(1, H, device=cuda).to(T)
    g1 = (1 + 0.1 * torch.randn(H, device=cuda)).to(T)
    # q|k|v: [3H, H] with the RMSNorm prologue
    wqkv = W(3 * H, H)
    got = ops.gemv(h, wqkv, norm_w=g1, eps=1e-5)
    assert _rel_err(got, rms(h, g1) @ wqkv.float().t()) < TOL[dt]
    _gemv_norm_check(got, h, wqkv, dt, g1, "q|k|v")
    # o_proj: [H, H] + residual
    a = torch.randn(1, H, device=cuda).to(T); wo = W(H, H)
    got = ops.gemv(a, wo, residual=h)
    assert _rel_err(got, a.float() @ wo.float().t() + h.float()) < TOL[dt]
    L.check(got, *L.linear_ref(a, wo, dt, residual=h)[:2], dt, "o_proj + residual")
    # in place on the residual stream, as the engine runs it
    h2 = h.clone(); ops.gemv(a, wo, residual=h2, out=h2)
    assert torch.equal(h2, got)
    # gate|up: [2I, H] interleaved, RMSNorm prologue + SiLU*mul epilogue
    wg, wu = W(I, H), W(I, H)
    fused = ops.interleave_gate_up(wg, wu)
    got = ops.gemv(h, fused, norm_w=g1, eps=1e-5, act=_C.ACT_SILU_MUL)
    xn = rms(h, g1)
    ref = torch.nn.functional.silu(xn @ wg.float().t()) * (xn @ wu.float().t())
    assert got.shape == (1, I) and _rel_err(got, ref) < TOL[dt]
    _gemv_norm_check(got, h, (wg, wu), dt, g1, "gate|up SiLU*mul", act=_C.ACT_SILU_MUL)
    # down_proj: [H, I] + residual
    act = torch.randn(1, I, device=cuda).to(T); wd = W(H, I)
    got = ops.gemv(act, wd, residual=h)
    assert _rel_err(got, act.float() @ wd.float().t() + h.float()) < TOL[dt]
    L.check(got, *L.linear_ref(act, wd, dt, residual=h)[:2], dt, "down_proj + residual")
    # lm_head: [32000, H] with the final norm
    wl = W(32000, H)
    got = ops.gemv(h, wl, norm_w=g1, eps=1e-5)
    assert _rel_err(got, rms(h, g1) @ wl.float().t()) < TOL[dt]
    _gemv_norm_check(got, h, wl, dt, g1, "lm_head")


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_norms(cuda, dt):
    from llava_mi355x import ops
    torch.manual_seed(3)
    x = (torch.randn(70, 1024, device=cuda) * 3 + 0.5).to(DT[dt])
    w = (1 + 0.1 * torch.randn(1024, device=cuda)).to(DT[dt]); b = (0.1 * torch.randn(1024, device=cuda)).to(DT[dt])
    xf = x.float()
    ref = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(DT[dt]).float() * w.float()
    assert _rel_err(ops.rmsnorm(x, w, 1e-5), ref) < TOL[dt]
    ref = torch.nn.functional.layer_norm(xf, (1024,), w.float(), b.float(), 1e-5)
    assert _rel_err(ops.layernorm(x, w, b, 1e-5), ref) < TOL[dt]


def _rope_table(n_pos, D, theta=10000.0):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2).float() / D))
    fr = torch.arange(n_pos).float()[:, None] * inv[None, :]
    return torch.cat([fr.cos(), fr.sin()], dim=-1).contiguous()      # [n_pos, D]: cos half | sin half


def _rope_ref(x, pos, table, D):
    # x [T, heads, D] fp32 ; HF rotate_half convention
    cos = torch.cat([table[pos, : D // 2]] * 2, -1)[:, None, :]
    sin = torch.cat([table[pos, D // 2:]] * 2, -1)[:, None, :]
    x1, x2 = x[..., : D // 2], x[..., D // 2:]
    return x * cos + torch.cat([-x2, x1], -1) * sin


@pytest.mark.parametrize("dt", ["bf16", "f32"])
@pytest.mark.parametrize("D,nh,nkv", [(128, 4, 4), (64, 4, 2)])
def test_rope_kv(cuda, dt, D, nh, nkv):
    from llava_mi355x import ops
    torch.manual_seed(1)
    T, pos0, s_max = 150, 37, 256
    qkv = torch.randn(T, (nh + 2 * nkv) * D, device=cuda).to(DT[dt])
    table = _rope_table(s_max, D).to(cuda)
    k, vt = ops.alloc_kv(nkv, s_max, D, DT[dt])
    src = qkv.clone()
    ops.rope_kv(qkv, k, vt, table, pos0, nh, nkv, D)
    pos = torch.arange(pos0, pos0 + T, device=cuda)
    q_ref = _rope_ref(src[:, : nh * D].float().view(T, nh, D), pos, table, D)
    k_ref = _rope_ref(src[:, nh * D:(nh + nkv) * D].float().view(T, nkv, D), pos, table, D)
    v_ref = src[:, (nh + nkv) * D:].float().view(T, nkv, D)
    assert _rel_err(qkv[:, : nh * D].view(T, nh, D), q_ref) < TOL[dt]
    assert _rel_err(k[:, pos0:pos0 + T].permute(1, 0, 2), k_ref) < TOL[dt]
    assert torch.equal(vt[:, :, pos0:pos0 + T].permute(2, 0, 1).float().cpu(), v_ref.cpu())
    assert k[:, :pos0].abs().sum() == 0 and k[:, pos0 + T:].abs().sum() == 0       # nothing outside the window touched


def _attn_ref(q, k, v, causal, q_pos0):
    # q [Tq, nh, D], k/v [Tk, nkv, D] fp32
    Tq, nh, D = q.shape
    nkv = k.shape[1]
    k = k.repeat_interleave(nh // nkv, dim=1); v = v.repeat_interleave(nh // nkv, dim=1)
    s = torch.einsum("qhd,khd->hqk", q, k) / math.sqrt(D)
    if causal:
        qi = torch.arange(Tq, device=q.device)[:, None] + q_pos0
        ki = torch.arange(k.shape[0], device=q.device)[None, :]
        s = s.masked_fill(ki > qi, float("-inf"))
    p = torch.softmax(s, dim=-1)
    return torch.einsum("hqk,khd->qhd", p, v)


def _fill_cache(k, v, s_max, dt, device):
    from llava_mi355x import ops
    Tk, nkv, D = k.shape
    kc, vt = ops.alloc_kv(nkv, s_max, D, dt, device)
    kc[:, :Tk] = k.permute(1, 0, 2).to(dt)
    vt[:, :, :Tk] = v.permute(1, 2, 0).to(dt)
    return kc, vt


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("D,nh,nkv,Tq,past,causal", [
    (128, 4, 4, 1087, 0, True), (128, 4, 2, 200, 300, True), (128, 2, 2, 64, 0, True), (128, 2, 2, 1, 77, True),
    (64, 4, 4, 577, 0, False), (64, 2, 2, 50, 0, False), (64, 2, 2, 130, 0, True)])
def test_flash_attn(cuda, dt, D, nh, nkv, Tq, past, causal):
    from llava_mi355x import ops
    torch.manual_seed(Tq + D)
    Tk = past + Tq
    s_max = ((Tk + 63) // 64) * 64 + 64
    q = torch.randn(Tq, nh, D, device=cuda).to(DT[dt]); k = torch.randn(Tk, nkv, D, device=cuda).to(DT[dt]); v = torch.randn(Tk, nkv, D, device=cuda).to(DT[dt])
    kc, vt = _fill_cache(k, v, s_max, DT[dt], cuda)
    got = ops.flash_attn(q.view(Tq, nh * D), kc, vt, Tq, Tk, past, nh, nkv, D, causal)
    ref = _attn_ref(q.float(), k.float(), v.float(), causal, past).reshape(Tq, nh * D)
    assert _rel_err(got, ref) < TOL[dt]


def test_flash_attn_real_shape_vs_fp32_and_hf_rounding_chain(cuda):
    """The prefill attention of the headline request: 32 heads x 128, 1087 positions, causal, bf16 (pin the MFMA / flash path at the
    real shape against the fp32 result, not only end to end).  Two references computed in fp64 / torch on the same bf16 inputs:
      * exact softmax(QK^T / sqrt d) V in fp64, rounded ONCE to bf16;
      * the reference's own bf16 chain (HF LlamaAttention: scores rounded to bf16, fp32 softmax cast to bf16, P.V with fp32 accumulation, rounded).
    The kernel keeps scores in fp32 and rounds only P (the MFMA operand) and the output, so it must be at least as close to the exact result as the
    reference's chain is (measured: 2.2x closer, max 8.3e-3 vs 1.9e-2, rms 2.5e-4 vs 5.4e-4) and inside the rounding-error bound of P at every element."""
    from llava_mi355x import ops
    torch.manual_seed(7)
    D, nh, T = 128, 32, 1087
    q = torch.randn(T, nh, D, device=cuda).bfloat16(); k = torch.randn(T, nh, D, device=cuda).bfloat16(); v = torch.randn(T, nh, D, device=cuda).bfloat16()
    kc, vt = _fill_cache(k, v, 1152, torch.bfloat16, cuda)
    got = ops.flash_attn(q.view(T, nh * D), kc, vt, T, T, 0, nh, nh, D, True).float().view(T, nh, D)
    exact = _attn_ref(q.double(), k.double(), v.double(), True, 0)
    once = exact.float().bfloat16().float()
    # HF chain: bf16 matmul output, scale in bf16, fp32 softmax -> bf16, bf16 matmul
    s = (torch.einsum("qhd,khd->hqk", q.float(), k.float()).bfloat16().float() / math.sqrt(D)).bfloat16().float()
    causal = torch.arange(T, device=cuda)[None, :] > torch.arange(T, device=cuda)[:, None]
    s = s.masked_fill(causal[None], torch.finfo(torch.bfloat16).min)
    p = torch.softmax(s, dim=-1).bfloat16().float()
    hf = torch.einsum("hqk,khd->qhd", p, v.float()).bfloat16().float()
    ulp = lambda x: torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - 7)          # bf16: 8 significant bits
    err_k = (got - exact.float()).abs(); err_hf = (hf - exact.float()).abs()
    print({"kernel_max_abs": err_k.max().item(), "hf_chain_max_abs": err_hf.max().item(), "kernel_rms": err_k.pow(2).mean().sqrt().item(),
           "hf_chain_rms": err_hf.pow(2).mean().sqrt().item()})
    assert err_k.pow(2).mean().sqrt().item() <= err_hf.pow(2).mean().sqrt().item()
    assert err_k.max().item() <= err_hf.max().item() * 1.05 + 1e-6
    # elementwise bound: P is rounded to bf16 before the P.V product (2^-9 relative per probability, numerator and denominator), the output once
    # more: |error| <= 2^-8 * sum_j p_ij |v_jd| + one output ulp — checked for every element (measured maximum 8.3e-3 at |v| up to 4.5)
    kk = k.double(); qq = q.double()
    sc = torch.einsum("qhd,khd->hqk", qq, kk) / math.sqrt(D)
    pe = torch.softmax(sc.masked_fill(causal[None], float("-inf")), dim=-1)
    mag = torch.einsum("hqk,khd->qhd", pe, v.double().abs()).float()
    assert ((got - exact.float()).abs() <= mag * 2.0 ** -8 + ulp(once)).all()


def test_flash_attn_forced_rescale(cuda):
    """A late key with a huge score forces the online-softmax rescale branch on every row (guide rule 26)."""
    from llava_mi355x import ops
    torch.manual_seed(0)
    D, nh, Tq = 128, 2, 256
    q = torch.randn(Tq, nh, D, device=cuda); k = torch.randn(Tq, nh, D, device=cuda) * 0.1; v = torch.randn(Tq, nh, D, device=cuda)
    k[200] = q[220] * 4.0     # spikes for rows >= 200 in the 4th key tile
    qb, kb, vb = q.bfloat16(), k.bfloat16(), v.bfloat16()
    kc, vt = _fill_cache(kb, vb, 320, torch.bfloat16, cuda)
    got = ops.flash_attn(qb.view(Tq, nh * D), kc, vt, Tq, Tq, 0, nh, nh, D, True)
    ref = _attn_ref(qb.float(), kb.float(), vb.float(), True, 0).reshape(Tq, nh * D)
    assert _rel_err(got, ref) < TOL["bf16"]


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("D,nh,nkv,rows,past,causal,n_split", [
    (128, 4, 4, 1, 1100, True, 8), (128, 4, 2, 1, 5, True, 8), (128, 2, 2, 40, 30, True, 1), (64, 4, 4, 33, 0, False, 1), (64, 2, 1, 1, 700, True, 4)])
def test_decode_attn(cuda, dt, D, nh, nkv, rows, past, causal, n_split):
    from llava_mi355x import ops
    torch.manual_seed(rows + past)
    Tk = past + rows if causal else 577
    s_max = ((Tk + 63) // 64) * 64 + 64
    q = torch.randn(rows, nh, D, device=cuda).to(DT[dt]); k = torch.randn(Tk, nkv, D, device=cuda).to(DT[dt]); v = torch.randn(Tk, nkv, D, device=cuda).to(DT[dt])
    kc, vt = _fill_cache(k, v, s_max, DT[dt], cuda)
    got = ops.decode_attn(q.view(rows, nh * D), kc, vt, rows, past, Tk, nh, nkv, D, causal, n_split=n_split)
    ref = _attn_ref(q.float(), k.float(), v.float(), causal, past).reshape(rows, nh * D)
    assert _rel_err(got, ref) < TOL[dt]


# decode_attn_step_kernel — the decode step's attention launch of 16-bit models — against float64 at the headline geometry (32 heads x 128) and the contexts the
# bench walks (1087 = first decode step, 1215 = last, 2047 = the cache's last slot): RoPE of q / k_new with HF's rounding points (cos / sin and the two products
# rounded to the model dtype), K / V^T append at `pos`, softmax(q K^T / sqrt(d)) V over keys 0..pos.
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nh,nkv,D,pos", [(32, 32, 128, 1087), (32, 32, 128, 1215), (32, 32, 128, 2047), (40, 40, 128, 1087), (32, 8, 128, 300), (16, 16, 64, 129), (4, 4, 128, 0)])
def test_decode_attn_step_vs_fp64(cuda, dt, nh, nkv, D, pos):
    from llava_mi355x import ops
    torch.manual_seed(pos + nh)
    T = DT[dt]
    s_max = 2048
    table = _rope_table(s_max, D).to(cuda)
    k_past = torch.randn(pos, nkv, D, device=cuda).to(T); v_past = torch.randn(pos, nkv, D, device=cuda).to(T)
    kc, vt = _fill_cache(k_past, v_past, s_max, T, cuda)
    qkv = torch.randn((nh + 2 * nkv) * D, device=cuda).to(T)
    src = qkv.clone()
    out = ops.decode_attn_step(qkv, kc, vt, table, pos, nh, nkv, D)
    # float64 statement
    p1 = torch.tensor([pos], device=cuda)
    tb = table.to(T).double()                                        # HF: cos / sin in the model dtype
    q_r = _rope_ref(src[: nh * D].double().view(1, nh, D), p1, tb, D).to(T)
    k_r = _rope_ref(src[nh * D:(nh + nkv) * D].double().view(1, nkv, D), p1, tb, D).to(T)
    v_n = src[(nh + nkv) * D:].view(1, nkv, D)
    k_all = torch.cat([k_past, k_r], 0).double(); v_all = torch.cat([v_past, v_n], 0).double()
    ref = _attn_ref(q_r.double(), k_all, v_all, False, 0).reshape(nh * D)
    assert _rel_err(out, ref) < TOL[dt]
    # element by element: ulp_T(ref) + the fp32 bound derived in forward_ref.py (the max-norm above measures late, small outputs against the largest one)
    R, k_chain, _, _ = FR.step_ref(src, k_past, v_past, table, pos, nh, nkv, D, dt)
    FR.check(out.view(1, nh, D), R.ref, R.step_bound(pos // 128 + 1), dt, f"decode_attn_step pos {pos}")
    # the append: the rotated k row is HF's chain T(T(x c) + T(r s)) bit for bit, the v column at `pos` exact; nothing else moved
    FR.exact_equal(kc[:, pos], k_chain, "appended key")
    assert torch.equal(vt[:, :, pos], v_n[0])
    assert torch.equal(kc[:, :pos], k_past.permute(1, 0, 2)) and (pos + 1 >= s_max or kc[:, pos + 1:].abs().sum() == 0)
    # run to run: the split-chunk merge is order-fixed
    kc2, vt2 = _fill_cache(k_past, v_past, s_max, T, cuda)
    out2 = ops.decode_attn_step(src.clone(), kc2, vt2, table, pos, nh, nkv, D)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("nh,nkv,D,K,pos", [(32, 32, 128, 4096, 1087), (32, 32, 128, 4096, 1215), (32, 32, 128, 4096, 2047), (40, 40, 128, 5120, 1150), (32, 8, 128, 4096, 300),
                                            (16, 16, 64, 1024, 129), (4, 4, 128, 512, 0), (4, 4, 128, 512, 127), (4, 4, 128, 512, 128), (8, 8, 64, 512, 383), (4, 2, 128, 1536, 63)])
def test_decode_kv_attn_is_bit_identical_to_projection_plus_attention(cuda, dt, nh, nkv, D, K, pos):
    """The split-q decode step's second launch (decode_kv_attn_kernel: the k | v projection next to the attention workgroups, the newest key / value handed over
    INSIDE the launch as tagged granules) against the two launches it replaces (q|k|v GEMV with the RMSNorm fused + decode_attn_step_kernel): same output row,
    same K / V^T append, bit for bit — headline widths of 7B / 13B, GQA, head_dim 64, the newest key first / last in its chunk, an empty cache.  The granule
    buffer is REUSED with a new tag and a different input row: values of the earlier launch (stale tags) must never be taken."""
    from llava_mi355x import ops
    torch.manual_seed(pos + 3 * nh)
    T = DT[dt]
    s_max = 2048
    table = _rope_table(s_max, D).to(cuda)
    k_past = torch.randn(pos, nkv, D, device=cuda).to(T); v_past = torch.randn(pos, nkv, D, device=cuda).to(T)
    w = (torch.randn((nh + 2 * nkv) * D, K, device=cuda) / K ** 0.5).to(T)
    g = (1 + 0.1 * torch.randn(K, device=cuda)).to(T)
    gran = torch.zeros(2 * nkv * D, dtype=torch.int64, device=cuda)
    for it, norm in enumerate((g, None, g)):
        x = torch.randn(1, K, device=cuda).to(T)
        row = ops.gemv(x, w, norm_w=norm, eps=1e-5)[0]                   # q | k | v, pre-RoPE
        kc, vt = _fill_cache(k_past, v_past, s_max, T, cuda)
        ref = ops.decode_attn_step(row.clone(), kc, vt, table, pos, nh, nkv, D)
        q_row = row.clone(); q_row[nh * D:] = float("nan")              # the k | v columns of the row are not to be read
        kc2, vt2 = _fill_cache(k_past, v_past, s_max, T, cuda)
        got = ops.decode_kv_attn(q_row, x[0], w[nh * D:], norm, 1e-5, kc2, vt2, table, pos, nh, nkv, D, granules=gran, tag=7 + it)
        assert torch.equal(got, ref), (it, (got.float() - ref.float()).abs().max().item())
        assert torch.equal(kc2, kc) and torch.equal(vt2, vt)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_argmax_first_index_wins(cuda, dt):
    from llava_mi355x import ops
    torch.manual_seed(2)
    x = torch.randn(32000, device=cuda).to(DT[dt])
    assert ops.argmax(x).item() == torch.argmax(x.float()).item()
    x[:] = 0; x[31999] = 5; x[17] = 5; x[4000] = 5
    assert ops.argmax(x).item() == 17


def test_im2col_matches_conv(cuda):
    from llava_mi355x import ops
    torch.manual_seed(4)
    pix = torch.randn(2, 3, 56, 56, device=cuda)
    w = torch.randn(32, 3, 14, 14, device=cuda)
    cols = ops.im2col(pix, 14, 640)
    assert cols[:, 588:].abs().sum() == 0
    got = cols[:, :588] @ w.view(32, -1).t()
    ref = torch.nn.functional.conv2d(pix, w, stride=14).flatten(2).transpose(1, 2).reshape(-1, 32)
    assert _rel_err(got, ref) < 1e-5
