"""A dtype code outside the table is an error at every single-op entry of the C ABI, never an fp32 (or fp16) run over the caller's buffers
(csrc/dispatch.h: dispatch_dtype / dispatch_dtype16).

The calls go to llava_mi355x._C.lib directly: llava_mi355x.ops maps torch dtypes and cannot produce a bad code.  Per entry: codes 3 and -1 (and 0 for the
entries that exist for the 16-bit types only) with otherwise valid arguments at the smallest legal shape must return non-zero, name the launcher and
"dtype" in lmx_last_error(), and leave the output buffer — prefilled with a bit pattern — untouched; the same call with a valid code then succeeds.
Every buffer is allocated as float32 of the ELEMENT count, so even an accidental fp32 interpretation would stay in bounds.  The error is raised on the
host before any launch, so each case is a few host calls.

Not here: lmx_op_gemm_qkv_rope.  Its entry asks gemm_fuses_qkv(dtype, ...) first, a pure predicate that is false for every code but 1 and 2, and reports "this shape
does not take the fused launch" before a launcher is reached; its smallest legal shape is also 160 tiles of 256 x 256.  lmx_op_preprocess needs a model handle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = 0, 1, 2
SENTINEL = 0x5A5A5A5A
D, S_MAX, H, V = 64, 128, 64, 64
EPS, SCALE = 1e-5, 0.125


def _C():
    from llava_mi355x import _C as C
    return C


def _buf(n):
    """n float32 elements of the sentinel pattern (an output, or an input whose values do not matter)."""
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _zeros(n, dtype):
    return torch.zeros(n, dtype=dtype, device="cuda")


class Case:
    """One entry: `make()` returns (output buffer, call) where call(dtype_code) -> status; `who` must appear in the message; `only16` adds code 0."""

    def __init__(self, name, who, make, only16=False, valid=BF16):
        self.name, self.who, self.make, self.only16, self.valid = name, who, make, only16, valid


def _p(t):
    return _C().ptr(t) if t is not None else None


def _st():
    return _C().stream_handle()


def _mk_rmsnorm():
    x, w, y = _buf(2 * H), _buf(H), _buf(2 * H)
    return y, lambda dt: _C().lib.lmx_op_rmsnorm(dt, _p(x), _p(w), _p(y), 2, H, EPS, _st()), (x, w)


def _mk_layernorm():
    x, w, b, y = _buf(2 * H), _buf(H), _buf(H), _buf(2 * H)
    return y, lambda dt: _C().lib.lmx_op_layernorm(dt, _p(x), _p(w), _p(b), _p(y), 2, H, EPS, _st()), (x, w, b)


def _mk_argmax():
    x = _buf(V)
    out = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    return out, lambda dt: _C().lib.lmx_op_argmax(dt, _p(x), V, _p(out), _st()), (x,)


def _mk_im2col():
    pix, out = _buf(3 * 4 * 4), _buf(4 * 16)
    return out, lambda dt: _C().lib.lmx_op_im2col(dt, _p(pix), _p(out), 1, 4, 2, 16, _st()), (pix,)


def _mk_gemv():
    x, w, c = _buf(H), _buf(64 * H), _buf(64)
    return c, lambda dt: _C().lib.lmx_op_gemv(dt, _p(x), _p(w), _p(c), None, None, None, EPS, 1, 64, H, H, H, 64, 0, 0, _st()), (x, w)


def _mk_gemm(variant, K):
    def make():
        x, w, c = _buf(2 * K), _buf(64 * K), _buf(2 * 64)
        return c, lambda dt: _C().lib.lmx_op_gemm(dt, _p(x), _p(w), _p(c), None, None, 2, 64, K, K, K, 64, 0, 0, variant, _st()), (x, w)
    return make


def _mk_rope_kv(entry):
    def make():
        qkv, kc, vt, cs = _buf(3 * D), _buf(S_MAX * D), _buf(S_MAX * D), _zeros(D, torch.float32)
        return kc, lambda dt: getattr(_C().lib, entry)(dt, D, _p(qkv), _p(kc), _p(vt), _p(cs), 0, 1, 1, 1, S_MAX, _st()), (qkv, vt, cs)
    return make


def _mk_flash():
    q, o, kc, vt = _buf(D), _buf(D), _buf(S_MAX * D), _buf(S_MAX * D)
    return o, lambda dt: _C().lib.lmx_op_flash_attn(dt, D, _p(q), _p(o), _p(kc), _p(vt), 1, 1, 0, D, D, 1, 1, S_MAX, SCALE, 1, _st()), (q, kc, vt)


def _mk_flash_lse():
    q, o, kc, vt, lse = _buf(D), _buf(D), _buf(S_MAX * D), _buf(S_MAX * D), _buf(64)
    return o, lambda dt: _C().lib.lmx_op_flash_attn_lse(dt, D, _p(q), _p(o), _p(kc), _p(vt), 1, 1, 0, D, D, 1, 1, S_MAX, SCALE, 1, _p(lse), 64, _st()), (q, kc, vt, lse)


def _mk_decode_attn():
    q, o, kc, vt, ws = _buf(D), _buf(D), _buf(S_MAX * D), _buf(S_MAX * D), _buf(D + 2)
    return o, lambda dt: _C().lib.lmx_op_decode_attn(dt, D, _p(q), _p(o), _p(kc), _p(vt), 1, 0, 1, 1, D, D, 1, 1, S_MAX, 1, SCALE, _p(ws), _st()), (q, kc, vt)


def _mk_decode_attn_step():
    qkv, kc, vt, cs, ws, out = _buf(3 * D), _buf(S_MAX * D), _buf(S_MAX * D), _zeros(D, torch.float32), _buf(D + 4), _buf(D)
    cnt = _zeros(1, torch.int32)
    return out, lambda dt: _C().lib.lmx_op_decode_attn_step(dt, D, _p(qkv), _p(kc), _p(vt), _p(cs), 0, 1, 1, S_MAX, SCALE, _p(ws), _p(cnt), _p(out), _st()), (qkv, cs)


def _mk_decode_fused():
    qkv, kc, vt, cs, ws, out = _buf(3 * D), _buf(S_MAX * D), _buf(S_MAX * D), _zeros(D, torch.float32), _buf(D + 4), _buf(D)
    pos, cnt = _zeros(1, torch.int32), _zeros(1, torch.int32)
    return out, lambda dt: _C().lib.lmx_op_decode_fused(dt, D, _p(qkv), _p(kc), _p(vt), _p(cs), _p(pos), 1, 1, S_MAX, SCALE, _p(ws), _p(cnt), _p(out), 0, _st()), (qkv, cs, pos)


def _mk_decode_attn_batch():
    import ctypes
    qkv, kc, vt, cs, ws, out = _buf(3 * D), _buf(S_MAX * D), _buf(S_MAX * D), _zeros(D, torch.float32), _buf(D + 4), _buf(D)
    pos, cnt = _zeros(1, torch.int32), _zeros(1, torch.int32)
    tab = torch.zeros(int(_C().lib.lmx_op_decode_attn_batch_tab_bytes(1)), dtype=torch.uint8, device="cuda")
    arr = lambda t: (ctypes.c_void_p * 1)(_p(t))
    return out, lambda dt: _C().lib.lmx_op_decode_attn_batch(dt, D, _p(qkv), 3 * D, arr(kc), arr(vt), arr(pos), arr(ws), arr(cnt), 1, _p(cs), 1, 1, S_MAX, 1, SCALE,
                                                             _p(tab), _p(out), D, _st()), (qkv, cs, pos, tab)


def _mk_decode_kv_attn():
    K = 64                                                        # k | v projection [2 D][K]; granules: one {bits, tag} 8-byte word per projected element
    qkv, x, w, nw, kc, vt = _buf(3 * D), _buf(K), _buf(2 * D * K), _buf(K), _buf(S_MAX * D), _buf(S_MAX * D)
    cs, ws, out, gran, cnt = _zeros(D, torch.float32), _buf(D + 4), _buf(D), _zeros(2 * 2 * D, torch.float32), _zeros(1, torch.int32)
    return out, lambda dt: _C().lib.lmx_op_decode_kv_attn(dt, D, _p(qkv), _p(x), _p(w), _p(nw), EPS, K, K, _p(kc), _p(vt), _p(cs), 0, 1, 1, S_MAX, SCALE, _p(ws), _p(cnt),
                                                          _p(gran), 1, _p(out), None, _st()), (qkv, x, w, nw, cs)


def _mk_attn_bwd_lse():
    T = 64
    q, k, v, o, do, lse = (_zeros(T * D, torch.float32) for _ in range(6))
    dq, dk, dv = _buf(T * D), _buf(T * D), _buf(T * D)
    return dq, lambda dt: _C().lib.lmx_op_attn_bwd_lse(dt, D, _p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), T, _p(dq), _p(dk), _p(dv), T, 1, 1, D, D, D, D, SCALE,
                                                       _st()), (q, k, v, o, do, lse, dk, dv)


def _mk_attn_bwd():
    T = 2
    q, k, v, do = (_zeros(T * D, torch.float32) for _ in range(4))
    dq, dk32, dv32, dk, dv = (_buf(T * D) for _ in range(5))
    return dq, lambda dt: _C().lib.lmx_op_attn_bwd(dt, D, _p(q), _p(k), _p(v), _p(do), _p(dq), _p(dk32), _p(dv32), _p(dk), _p(dv), T, 1, 1, D, D, D, SCALE,
                                                   _st()), (q, k, v, do, dk32, dv32, dk, dv)


def _mk_elementwise():
    a, b, out = _buf(64), _buf(64), _buf(64)
    return out, lambda dt: _C().lib.lmx_op_elementwise(dt, 3, _p(a), _p(b), _p(out), 64, _st()), (a, b)


def _mk_cast_f32():
    src, dst = _zeros(64, torch.float32), _buf(64)
    return dst, lambda dt: _C().lib.lmx_op_cast_f32(dt, _p(src), _p(dst), 64, _st()), (src,)


def _mk_col_sum():
    dy, out = _buf(2 * 64), _buf(64)
    return out, lambda dt: _C().lib.lmx_op_col_sum(dt, _p(dy), 64, 2, 64, _p(out), _st()), (dy,)


def _mk_sumsq():
    x, acc = _buf(64), _buf(1)
    return acc, lambda dt: _C().lib.lmx_op_sumsq(dt, _p(x), 64, _p(acc), _st()), (x,)


def _mk_adamw():
    p, g, master, m, v = _buf(64), _buf(64), _zeros(64, torch.float32), _zeros(64, torch.float32), _zeros(64, torch.float32)
    return p, lambda dt: _C().lib.lmx_op_adamw(dt, _p(p), _p(g), _p(master), _p(m), _p(v), 64, 0.1, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, _st()), (g, master, m, v)


def _mk_swiglu_bwd():
    g, u, da, dg, du = (_buf(64) for _ in range(5))
    return dg, lambda dt: _C().lib.lmx_op_swiglu_bwd(dt, _p(g), _p(u), _p(da), _p(dg), _p(du), 64, _st()), (g, u, da, du)


def _mk_rope_bwd():
    dy, dx, cs = _buf(D), _buf(D), _zeros(D, torch.float32)
    return dx, lambda dt: _C().lib.lmx_op_rope_bwd(dt, _p(dy), _p(dx), _p(cs), 0, 1, 1, D, D, _st()), (dy, cs)


def _mk_transpose(rows, cols):
    """2 x 64: the scalar kernel; 8 x 8 with aligned pointers: the untyped 16-bit vector kernel, which every code but 0 used to reach."""
    def make():
        src, dst = _buf(rows * cols), _buf(cols * rows)
        return dst, lambda dt: _C().lib.lmx_op_transpose(dt, _p(src), cols, rows, cols, _p(dst), rows, _st()), (src,)
    return make


def _mk_gemm_wgrad():
    dy, x, out = _zeros(64 * 256, torch.float32), _zeros(64 * 256, torch.float32), _buf(256 * 256)
    return out, lambda dt: _C().lib.lmx_op_gemm_wgrad(dt, _p(dy), 256, _p(x), 256, 64, 256, 256, _p(out), 256, _st()), (dy, x)


def _mk_rmsnorm_bwd(with_res):
    def make():
        x, w, dy, res, dx, scratch = _buf(2 * H), _buf(H), _buf(2 * H), _buf(2 * H), _buf(2 * H), _buf(64 + H)
        if with_res:
            return dx, lambda dt: _C().lib.lmx_op_rmsnorm_bwd_add(dt, _p(x), _p(w), _p(dy), _p(res), _p(dx), None, _p(scratch), 2, H, EPS, _st()), (x, w, dy, res)
        return dx, lambda dt: _C().lib.lmx_op_rmsnorm_bwd(dt, _p(x), _p(w), _p(dy), _p(dx), None, _p(scratch), 2, H, EPS, _st()), (x, w, dy)
    return make


def _mk_ce_loss():
    logits, labels = _zeros(2 * V, torch.float32), _zeros(2, torch.int64)
    lse, row_loss, out2 = _buf(1), _buf(1), _buf(2)
    return out2, lambda dt: _C().lib.lmx_op_ce_loss(dt, _p(logits), V, _p(labels), 1, 2, V, -100, _p(lse), _p(row_loss), _p(out2), 1.0, None, 0, _st()), (logits, labels)


def _mk_gather_embed():
    src, table, out = _zeros(1, torch.int32), _buf(2 * H), _buf(H)
    return out, lambda dt: _C().lib.lmx_op_gather_embed(dt, _p(src), _p(table), None, _p(out), 1, H, _st()), (src, table)


def _mk_embed_bwd():
    src, d, dtable = _zeros(1, torch.int32), _zeros(H, torch.float32), _buf(2 * H)
    return dtable, lambda dt: _C().lib.lmx_op_embed_bwd(dt, _p(src), _p(d), _p(dtable), None, 1, H, _st()), (src, d)


def _mk_beam_topk():
    logits, scores, out_s = _zeros(V, torch.float32), _zeros(1, torch.float32), _buf(1)
    out_i = _zeros(1, torch.int32)
    return out_s, lambda dt: _C().lib.lmx_op_beam_topk(dt, _p(logits), V, V, 1, _p(scores), 1, _p(out_s), _p(out_i), _st()), (logits, scores)


def _mk_beam_sample_topk():
    logits, scores, out_k, out_s = _zeros(V, torch.float32), _zeros(1, torch.float32), _buf(1), _buf(1)
    out_i = _zeros(1, torch.int32)
    return out_k, lambda dt: _C().lib.lmx_op_beam_sample_topk(dt, _p(logits), V, V, 1, None, _p(scores), 1.0, 7, 0, 1, _p(out_k), _p(out_s), _p(out_i), _st()), (logits, scores)


def _mk_sample():
    logits, off = _zeros(V, torch.float32), _zeros(1, torch.int32)
    out = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    return out, lambda dt: _C().lib.lmx_op_sample(dt, _p(logits), V, 1.0, 1.0, 0, 7, _p(off), None, _p(out), None, _st()), (logits, off)


CASES = [
    Case("rmsnorm", "rmsnorm", _mk_rmsnorm),
    Case("layernorm", "layernorm", _mk_layernorm),
    Case("argmax", "argmax", _mk_argmax),
    Case("im2col", "im2col", _mk_im2col),
    Case("gemv", "gemv", _mk_gemv),
    Case("gemm", "gemm", _mk_gemm(0, 64)),
    Case("gemm_skinny20", "skinny_gemm", _mk_gemm(20, 128), only16=True),
    Case("gemm_skinny21", "skinny_swizzle", _mk_gemm(21, 128), only16=True),
    Case("rope_kv", "rope_kv", _mk_rope_kv("lmx_op_rope_kv")),
    Case("rope_kv_rows", "rope_kv", _mk_rope_kv("lmx_op_rope_kv_rows")),
    Case("flash_attn", "flash_prefill", _mk_flash, only16=True),
    Case("flash_attn_lse", "flash_prefill", _mk_flash_lse, only16=True),
    Case("decode_attn", "decode_attn", _mk_decode_attn),
    Case("decode_attn_step", "decode_attn_step", _mk_decode_attn_step, only16=True),
    Case("decode_fused", "decode_fused", _mk_decode_fused),
    Case("decode_attn_batch", "decode_fused", _mk_decode_attn_batch),
    Case("decode_kv_attn", "decode_kv_attn", _mk_decode_kv_attn, only16=True),
    # the entry's own check (capi.cpp) names the dtype before launch_attn_bwd_mfma is reached: that check, not the launcher's dispatch, is what this case covers
    Case("attn_bwd_lse", "attn_bwd_lse", _mk_attn_bwd_lse, only16=True),
    Case("attn_bwd", "attn_bwd", _mk_attn_bwd, valid=F32),
    Case("elementwise", "elementwise", _mk_elementwise),
    Case("cast_f32", "cast_f32", _mk_cast_f32),
    Case("col_sum", "col_sum", _mk_col_sum),
    Case("sumsq", "sumsq", _mk_sumsq),
    Case("adamw", "adamw", _mk_adamw),
    Case("swiglu_bwd", "swiglu_bwd", _mk_swiglu_bwd),
    Case("rope_bwd", "rope_bwd", _mk_rope_bwd),
    Case("transpose", "transpose", _mk_transpose(2, 64)),
    Case("transpose_vec", "transpose", _mk_transpose(8, 8)),
    Case("gemm_wgrad", "gemm_wgrad", _mk_gemm_wgrad, only16=True),
    Case("rmsnorm_bwd", "rmsnorm_bwd", _mk_rmsnorm_bwd(False)),
    Case("rmsnorm_bwd_add", "rmsnorm_bwd", _mk_rmsnorm_bwd(True)),
    Case("ce_loss", "ce_loss", _mk_ce_loss),
    Case("gather_embed", "gather_embed", _mk_gather_embed),
    Case("embed_bwd", "embed_bwd", _mk_embed_bwd),
    Case("beam_topk", "beam_topk", _mk_beam_topk),
    Case("beam_sample_topk", "beam_gumbel_topk", _mk_beam_sample_topk),
    Case("sample", "sample", _mk_sample),
]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bad_dtype_code_is_an_error_and_touches_nothing(case):
    C = _C()
    out, call, _inputs = case.make()
    before = out.clone()
    for code in (3, -1) + ((F32,) if case.only16 else ()):
        status = call(code)
        msg = C.last_error()
        assert status != 0, f"{case.name}: dtype code {code} was accepted"
        assert "dtype" in msg and case.who in msg, f"{case.name}: dtype code {code}: message {msg!r} names neither the dtype nor {case.who!r}"
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32) if out.dtype == torch.float32 else out, before.view(torch.int32) if before.dtype == torch.float32 else before), \
            f"{case.name}: dtype code {code} was refused but the output buffer changed"
    status = call(case.valid)
    assert status == 0, f"{case.name}: valid dtype code {case.valid} failed after the refused calls: {C.last_error()}"
    torch.cuda.synchronize()
