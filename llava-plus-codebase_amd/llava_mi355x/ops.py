"""Single-op wrappers over the C ABI (`lmx_op_*`): the same HIP kernels the engine launches, exposed for unit parity
tests and microbenchmarks.  torch tensors are containers only (pointers + current stream)."""
from __future__ import annotations

import math

import torch

from . import _C
from ._C import check, lib, ptr, stream_handle, torch_dtype_code


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("llava_mi355x ops need tensors on the MI355X (cuda) device; there is no CPU fallback")
        if t is not None and not t.is_contiguous():
            raise ValueError("llava_mi355x ops need contiguous tensors")


def _need_cuda_rows(*ts):
    """As _need_cuda for 2-D operands whose ROWS are contiguous but whose row stride is free (column windows of wider buffers): the entry point takes the stride."""
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("llava_mi355x ops need tensors on the MI355X (cuda) device; there is no CPU fallback")
        if t is not None and (t.dim() != 2 or t.stride(1) != 1):
            raise ValueError("llava_mi355x ops need 2-D operands with contiguous rows")


def gemm(x, w, bias=None, residual=None, act=_C.ACT_NONE, variant=0, out=None):
    """act(x @ w.T + bias) (+ residual).  x [M,K], w [N,K]; SiLU·mul expects w as the fused [32 gate|32 up] layout.  x, residual and out may be column windows
    of wider buffers (contiguous rows, free row stride: the entry point takes the strides); out may be the residual's own buffer."""
    _need_cuda(w, bias)
    _need_cuda_rows(x, residual, out)
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if act == _C.ACT_SILU_MUL else N
    if out is None:
        out = torch.empty((M, n_out), dtype=x.dtype, device=x.device)
    check(lib.lmx_op_gemm(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(out), ptr(bias), ptr(residual), M, N, K,
                          x.stride(0), w.stride(0), out.stride(0), residual.stride(0) if residual is not None else 0,
                          act, variant, stream_handle()), "gemm")
    return out


def gemv(x, w, bias=None, residual=None, norm_w=None, eps=1e-5, act=_C.ACT_NONE, out=None):
    """Decode-time linear for 1..4 rows: act(norm(x) @ w.T + bias) (+ residual).  x, w, residual and out may be column windows of wider buffers (contiguous
    rows, free row stride)."""
    _need_cuda(bias, norm_w)
    _need_cuda_rows(x, w, residual, out)
    MB, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if act == _C.ACT_SILU_MUL else N
    if out is None:
        out = torch.empty((MB, n_out), dtype=x.dtype, device=x.device)
    if w.shape[1] != K or tuple(out.shape) != (MB, n_out) or (residual is not None and tuple(residual.shape) != (MB, n_out)):
        raise ValueError("gemv: x [MB, K], w [N, K], residual / out [MB, N] (N / 2 for SiLU*mul)")
    check(lib.lmx_op_gemv(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(out), ptr(bias), ptr(residual), ptr(norm_w), eps,
                          MB, N, K, x.stride(0), w.stride(0), out.stride(0), residual.stride(0) if residual is not None else 0,
                          act, stream_handle()), "gemv")
    return out


def gemv_rot_pack(w, rot, norm=False, act=_C.ACT_NONE, rows_per_wave=None):
    """Rotated decode copy of a 16-bit weight w [N, K] (contiguous rows, free row stride) for gemv_rot with the same `norm` (an RMSNorm weight will be given) and
    `act`: [N, pitch] with pitch = whole 1-KiB load rounds, zero past K; physical round p of row n holds logical round (p - (n // R * rot) % NR) % NR.
    rows_per_wave: R of another reader (decode_kv_attn: 2); default: the single-row launch's own choice for the shape."""
    _need_cuda_rows(w)
    N, K = w.shape
    R = rows_per_wave if rows_per_wave is not None else lib.lmx_op_gemv_rot_rows(N, K, int(bool(norm)), act)
    out = torch.empty((N, lib.lmx_op_gemv_rot_pitch(K)), dtype=w.dtype, device=w.device)
    check(lib.lmx_op_gemv_rot_pack(torch_dtype_code(w.dtype), ptr(w), w.stride(0), ptr(out), N, K, R, int(rot), act, stream_handle()), "gemv_rot_pack")
    return out


def gemv_rot(x, w_rot, K, rot, bias=None, residual=None, norm_w=None, eps=1e-5, act=_C.ACT_NONE, out=None):
    """gemv(x [1, K], w) on the rotated copy w_rot = gemv_rot_pack(w, rot, norm=norm_w is not None, act=act): the same bits, the waves of the launch start
    their rows at different load rounds.  Shapes the hand-counted 16-bit stream does not take are an error."""
    _need_cuda(x, w_rot, bias, residual, norm_w)
    N = w_rot.shape[0]
    n_out = N // 2 if act == _C.ACT_SILU_MUL else N
    if out is None:
        out = torch.empty((1, n_out), dtype=x.dtype, device=x.device)
    if tuple(x.shape) != (1, K) or w_rot.shape[1] != lib.lmx_op_gemv_rot_pitch(K) or not w_rot.is_contiguous() or tuple(out.shape) != (1, n_out) \
            or (residual is not None and tuple(residual.shape) != (1, n_out)):
        raise ValueError("gemv_rot: x [1, K], w_rot [N, pitch(K)] contiguous, residual / out [1, N] (N / 2 for SiLU*mul)")
    check(lib.lmx_op_gemv_rot(torch_dtype_code(x.dtype), ptr(x), ptr(w_rot), ptr(out), ptr(bias), ptr(residual), ptr(norm_w), eps, N, K, act, int(rot),
                              stream_handle()), "gemv_rot")
    return out


def rmsnorm(x, w, eps):
    _need_cuda(x, w)
    y = torch.empty_like(x)
    check(lib.lmx_op_rmsnorm(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(y), x.shape[0], x.shape[1], eps, stream_handle()), "rmsnorm")
    return y


def layernorm(x, w, b, eps):
    _need_cuda(x, w, b)
    y = torch.empty_like(x)
    check(lib.lmx_op_layernorm(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(b), ptr(y), x.shape[0], x.shape[1], eps, stream_handle()), "layernorm")
    return y


def interleave_gate_up(gate, up):
    """Host-side statement of the fused [32 gate | 32 up] row layout the SiLU·mul epilogue expects (tests only;
    the engine does this on the device at weight-load time)."""
    I, K = gate.shape
    assert I % 32 == 0
    g = gate.view(I // 32, 32, K)
    u = up.view(I // 32, 32, K)
    return torch.cat([g, u], dim=1).reshape(2 * I, K).contiguous()


def alloc_kv(n_kv_heads, s_max, head_dim, dtype, device="cuda"):
    """Zero-initialised K cache [kvh][s_max][D] and Vᵀ cache [kvh][D][s_max] (one layer)."""
    k = torch.zeros((n_kv_heads, s_max, head_dim), dtype=dtype, device=device)
    vt = torch.zeros((n_kv_heads, head_dim, s_max), dtype=dtype, device=device)
    return k, vt


def rope_kv(qkv, kcache, vtcache, cos_sin, pos0, n_heads, n_kv_heads, head_dim, k_rows=False):
    """Rotate q in place, write rotated k rows and v columns into the caches at positions pos0..; k_rows: the rotated k also replaces the k columns of qkv."""
    _need_cuda(qkv, kcache, vtcache, cos_sin)
    T = qkv.shape[0]
    assert qkv.shape[1] == (n_heads + 2 * n_kv_heads) * head_dim
    s_max = kcache.shape[1]
    fn = lib.lmx_op_rope_kv_rows if k_rows else lib.lmx_op_rope_kv
    check(fn(torch_dtype_code(qkv.dtype), head_dim, ptr(qkv), ptr(kcache), ptr(vtcache), ptr(cos_sin), pos0, T, n_heads, n_kv_heads, s_max, stream_handle()), "rope_kv")


def gemm_qkv_rope(x, w, qkv, kcache, vtcache, cos_sin, pos0, n_heads, n_kv_heads, head_dim):
    """q|k|v projection with RoPE + KV append in the GEMM epilogue: rotated q into qkv[:, :n_heads*D], rotated k / v into the caches at pos0.."""
    _need_cuda(x, w, qkv, kcache, vtcache, cos_sin)
    T, K = x.shape
    assert w.shape == ((n_heads + 2 * n_kv_heads) * head_dim, K) and qkv.shape == (T, w.shape[0]) and x.is_contiguous() and w.is_contiguous() and qkv.is_contiguous()
    check(lib.lmx_op_gemm_qkv_rope(torch_dtype_code(x.dtype), head_dim, ptr(x), ptr(w), ptr(qkv), ptr(kcache), ptr(vtcache), ptr(cos_sin), pos0, T, K,
                                   n_heads, n_kv_heads, kcache.shape[1], stream_handle()), "gemm_qkv_rope")


def flash_attn(q, kcache, vtcache, q_len, kv_len, q_pos0, n_heads, n_kv_heads, head_dim, causal, q_stride=None, out=None, lse=None):
    """Prefill attention over the caches.  q: [q_len, q_stride] with head h at column h*D.  lse (optional, [n_heads, >= q_len] float32): receives the log2-domain
    log-sum-exp of every row's scaled scores — what attn_bwd_lse takes instead of recomputing it."""
    _need_cuda(q, kcache, vtcache, lse)
    if q_stride is None:
        q_stride = q.stride(0)
    if out is None:
        out = torch.empty((q_len, n_heads * head_dim), dtype=q.dtype, device=q.device)
    s_max = kcache.shape[1]
    if lse is not None:
        assert lse.dtype == torch.float32 and lse.shape[0] == n_heads and lse.shape[1] >= q_len
        check(lib.lmx_op_flash_attn_lse(torch_dtype_code(q.dtype), head_dim, ptr(q), ptr(out), ptr(kcache), ptr(vtcache), q_len, kv_len, q_pos0, q_stride, out.stride(0),
                                        n_heads, n_kv_heads, s_max, 1.0 / math.sqrt(head_dim), int(causal), ptr(lse), lse.stride(0), stream_handle()), "flash_attn_lse")
        return out
    check(lib.lmx_op_flash_attn(torch_dtype_code(q.dtype), head_dim, ptr(q), ptr(out), ptr(kcache), ptr(vtcache), q_len, kv_len, q_pos0,
                                q_stride, out.stride(0), n_heads, n_kv_heads, s_max, 1.0 / math.sqrt(head_dim), int(causal),
                                stream_handle()), "flash_attn")
    return out


def decode_attn(q, kcache, vtcache, n_rows, pos0, kv_total, n_heads, n_kv_heads, head_dim, causal, n_split=1, q_stride=None, out=None):
    _need_cuda(q, kcache, vtcache)
    if q_stride is None:
        q_stride = q.stride(0)
    if out is None:
        out = torch.empty((n_rows, n_heads * head_dim), dtype=q.dtype, device=q.device)
    s_max = kcache.shape[1]
    ws = torch.empty(lib.lmx_op_decode_attn_ws_bytes(n_rows, n_heads, n_split, head_dim) // 4, dtype=torch.float32, device=q.device)
    check(lib.lmx_op_decode_attn(torch_dtype_code(q.dtype), head_dim, ptr(q), ptr(out), ptr(kcache), ptr(vtcache), n_rows, pos0, kv_total,
                                 int(causal), q_stride, out.stride(0), n_heads, n_kv_heads, s_max, n_split, 1.0 / math.sqrt(head_dim),
                                 ptr(ws), stream_handle()), "decode_attn")
    return out


def decode_attn_scratch(n_heads, n_split, head_dim, dtype, device):
    """(partials workspace, zeroed arrival counters, output row) of the decode-step attention launches; reusable across launches (the merger re-arms the counters)"""
    return (torch.zeros(n_heads * n_split * (head_dim + 4), dtype=torch.float32, device=device), torch.zeros(n_heads, dtype=torch.int32, device=device),
            torch.empty(n_heads * head_dim, dtype=dtype, device=device))


def decode_attn_step(qkv, kcache, vtcache, cos_sin, pos, n_heads, n_kv_heads, head_dim, scratch=None):
    """The decode step's attention launch (16-bit models): RoPE(q, k_new) at `pos`, K / V^T append, attention over keys 0..pos.  qkv: one [q|k|v] row
    (pre-RoPE).  Returns the [n_heads * head_dim] output row."""
    _need_cuda(qkv, kcache, vtcache, cos_sin)
    s_max = kcache.shape[1]
    n_split = (s_max + 127) // 128
    ws, cnt, out = scratch if scratch is not None else decode_attn_scratch(n_heads, n_split, head_dim, qkv.dtype, qkv.device)
    check(lib.lmx_op_decode_attn_step(torch_dtype_code(qkv.dtype), head_dim, ptr(qkv), ptr(kcache), ptr(vtcache), ptr(cos_sin), int(pos), n_heads, n_kv_heads,
                                      s_max, 1.0 / (head_dim ** 0.5), ptr(ws), ptr(cnt), ptr(out), stream_handle()), "decode_attn_step")
    return out


def decode_fused(qkv, kcache, vtcache, cos_sin, pos, n_heads, n_kv_heads, head_dim, scratch=None):
    """The decode step's attention launch of fp32 models (decode_fused_kernel, one sequence): RoPE(q, k_new) at `pos` (an int, or the int32 [1] device position
    word the engine keeps), K / V^T append, attention over keys 0..pos in 128-key chunks merged by the last chunk to arrive.  qkv: one [q|k|v] row (pre-RoPE).
    Returns the [n_heads * head_dim] output row."""
    if not isinstance(pos, torch.Tensor):
        pos = torch.tensor([int(pos)], dtype=torch.int32, device=qkv.device)
    _need_cuda(qkv, kcache, vtcache, cos_sin, pos)
    assert pos.dtype == torch.int32 and pos.numel() == 1
    s_max = kcache.shape[1]
    n_split = (s_max + 127) // 128
    ws, cnt, out = scratch if scratch is not None else decode_attn_scratch(n_heads, n_split, head_dim, qkv.dtype, qkv.device)
    check(lib.lmx_op_decode_fused(torch_dtype_code(qkv.dtype), head_dim, ptr(qkv), ptr(kcache), ptr(vtcache), ptr(cos_sin), ptr(pos), n_heads, n_kv_heads,
                                  s_max, 1.0 / (head_dim ** 0.5), ptr(ws), ptr(cnt), ptr(out), 0, stream_handle()), "decode_fused")
    return out


def decode_attn_batch(qkv, kcaches, vtcaches, pos_words, cos_sin, n_heads, n_kv_heads, head_dim, n_split=None, out=None):
    """The decode BATCH's attention launch (continuous batching): row z of qkv [n_seq, (n_heads + 2 n_kv_heads) head_dim] (pre-RoPE) against sequence z's own
    caches kcaches[z] [n_kv_heads, s_max, D] / vtcaches[z] [n_kv_heads, D, s_max] and its device position word pos_words[z] (int32 [1]: keys already cached).
    Appends the rotated key / the value at that position and returns the [n_seq, n_heads * head_dim] attention rows (into `out` when given: rows may be a
    column window of a wider buffer)."""
    import ctypes
    n_seq = qkv.shape[0]
    _need_cuda(qkv, cos_sin, *kcaches, *vtcaches, *pos_words)
    assert len(kcaches) == len(vtcaches) == len(pos_words) == n_seq and qkv.stride(1) == 1
    s_max = kcaches[0].shape[1]
    if n_split is None:
        n_split = (s_max + 127) // 128
    arr = lambda ts: (ctypes.c_void_p * n_seq)(*[ptr(t) for t in ts])
    ws = [torch.zeros(n_heads * n_split * (head_dim + 4), dtype=torch.float32, device=qkv.device) for _ in range(n_seq)]
    cnt = [torch.zeros(n_heads, dtype=torch.int32, device=qkv.device) for _ in range(n_seq)]
    tab = torch.empty(int(lib.lmx_op_decode_attn_batch_tab_bytes(n_seq)), dtype=torch.uint8, device=qkv.device)
    if out is None:
        out = torch.empty(n_seq, n_heads * head_dim, dtype=qkv.dtype, device=qkv.device)
    assert out.shape == (n_seq, n_heads * head_dim) and out.stride(1) == 1
    check(lib.lmx_op_decode_attn_batch(torch_dtype_code(qkv.dtype), head_dim, ptr(qkv), qkv.stride(0), arr(kcaches), arr(vtcaches), arr(pos_words), arr(ws), arr(cnt),
                                       n_seq, ptr(cos_sin), n_heads, n_kv_heads, s_max, int(n_split), 1.0 / (head_dim ** 0.5), ptr(tab), ptr(out), out.stride(0),
                                       stream_handle()), "decode_attn_batch")
    return out


def decode_kv_attn(q_row, x, w_kv, norm_w, eps, kcache, vtcache, cos_sin, pos, n_heads, n_kv_heads, head_dim, granules=None, tag=1, timeline=None, scratch=None, rot=0):
    """The split-q decode step's second launch: the k | v projection of the (RMS-normalised, when norm_w is given) input row x next to the attention
    workgroups.  q_row: a [q|k|v]-sized row whose q columns hold the pre-RoPE query (the k | v columns are ignored).  Same effects as gemv + decode_attn_step.
    rot > 0: w_kv is gemv_rot_pack(k | v rows, rot, rows_per_wave=2), the rotated copy."""
    _need_cuda(q_row, x, w_kv, kcache, vtcache, cos_sin)
    s_max = kcache.shape[1]
    n_split = (s_max + 127) // 128
    ws, cnt, out = scratch if scratch is not None else decode_attn_scratch(n_heads, n_split, head_dim, x.dtype, x.device)
    if granules is None:
        granules = torch.zeros(2 * n_kv_heads * head_dim, dtype=torch.int64, device=x.device)
    if rot:
        if w_kv.shape[1] != lib.lmx_op_gemv_rot_pitch(x.shape[-1]) or not w_kv.is_contiguous():
            raise ValueError("decode_kv_attn: a rotated copy is [2 * n_kv_heads * head_dim, pitch(K)] contiguous")
        check(lib.lmx_op_decode_kv_attn_rot(torch_dtype_code(x.dtype), head_dim, ptr(q_row), ptr(x), ptr(w_kv), ptr(norm_w), float(eps), x.shape[-1], int(rot),
                                            ptr(kcache), ptr(vtcache), ptr(cos_sin), int(pos), n_heads, n_kv_heads, s_max, 1.0 / (head_dim ** 0.5), ptr(ws), ptr(cnt),
                                            ptr(granules), int(tag), ptr(out), ptr(timeline), stream_handle()), "decode_kv_attn_rot")
        return out
    check(lib.lmx_op_decode_kv_attn(torch_dtype_code(x.dtype), head_dim, ptr(q_row), ptr(x), ptr(w_kv), ptr(norm_w), float(eps), x.shape[-1], w_kv.stride(0),
                                    ptr(kcache), ptr(vtcache), ptr(cos_sin), int(pos), n_heads, n_kv_heads, s_max, 1.0 / (head_dim ** 0.5), ptr(ws), ptr(cnt),
                                    ptr(granules), int(tag), ptr(out), ptr(timeline), stream_handle()), "decode_kv_attn")
    return out


def argmax(logits):
    _need_cuda(logits)
    out = torch.zeros(1, dtype=torch.int64, device=logits.device)
    check(lib.lmx_op_argmax(torch_dtype_code(logits.dtype), ptr(logits), logits.numel(), ptr(out), stream_handle()), "argmax")
    return out


def score_row(buf, V, history=(), n_out=0, token=-1, penalty=1.0, ngram=0, min_new=0, eos=(), suppress=(), temperature=0.0, top_p=1.0, top_k=0, seed=0,
              u32=None, want_row=True):
    """The score recorder (csrc/sampling.hip, lmx_op_score_row) on one row: `buf` is a device buffer of ld = buf.numel() >= V elements whose first V are the
    raw logits; `history` the ids the logits processors see, the last n_out of them generated.  temperature <= 0: the greedy row, else the sampled one
    (u32: the uniform number as a 32-bit integer, else Philox(seed, n_out)).  token < 0 (sampled only): score the id re-drawn under that number.
    Returns (processed fp32 row [V] or None, lse, logprob, re-drawn id or -1) — the row on the device, the scalars as Python numbers."""
    import ctypes
    _need_cuda(buf)
    dev = buf.device
    hist = [int(t) for t in history]
    h = torch.tensor(hist or [0], dtype=torch.long, device=dev)
    eos, sup = [int(t) for t in eos], [int(t) for t in suppress]
    e = (ctypes.c_int64 * max(1, len(eos)))(*eos)
    s = (ctypes.c_int64 * max(1, len(sup)))(*sup)
    row = torch.empty(V, dtype=torch.float32, device=dev) if want_row else None
    out2 = torch.zeros(2, dtype=torch.float32, device=dev)
    redraw = torch.full((1,), -1, dtype=torch.long, device=dev)
    keep = torch.zeros(V, dtype=torch.uint8, device=dev) if temperature > 0 else None
    uo = ctypes.pointer(ctypes.c_uint32(int(u32))) if u32 is not None else None
    check(lib.lmx_op_score_row(torch_dtype_code(buf.dtype), ptr(buf), int(V), buf.numel(), ptr(h), len(hist), int(n_out), float(penalty), int(ngram), int(min_new),
                               e, len(eos), s, len(sup), float(temperature), float(top_p), int(top_k), int(seed), uo, int(token), ptr(row), ptr(out2), ptr(redraw),
                               ptr(keep), stream_handle()), "score_row")
    lse, lp = out2.tolist()
    return row, lse, lp, int(redraw.item())


def im2col(pixels, patch, kpad):
    _need_cuda(pixels)
    N, C, S, _ = pixels.shape
    P = (S // patch) ** 2
    out = torch.empty((N * P, kpad), dtype=pixels.dtype, device=pixels.device)
    check(lib.lmx_op_im2col(torch_dtype_code(pixels.dtype), ptr(pixels), ptr(out), N, S, patch, kpad, stream_handle()), "im2col")
    return out


# ---- training-step slices (csrc/train.hip) -----------------------------------------------------------------------------------------
def ce_loss(logits, labels, ignore_index=-100, want_grad=False, grad=1.0):
    """Shifted cross-entropy of LlamaForCausalLM.forward: logits [B,T,V] (model dtype), labels [B,T] int64 -> (loss fp32 scalar tensor,
    counted positions, dlogits | None).  Mean over positions whose label (at t+1) is not ignore_index; fp32 math on the stored logits."""
    _need_cuda(logits, labels)
    B, T, V = logits.shape
    R = B * (T - 1)
    lse = torch.empty(R, dtype=torch.float32, device=logits.device); row = torch.empty_like(lse)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    d = torch.empty_like(logits) if want_grad else None
    check(lib.lmx_op_ce_loss(torch_dtype_code(logits.dtype), ptr(logits), logits.stride(1), ptr(labels), B, T, V, int(ignore_index), ptr(lse), ptr(row),
                             ptr(out), float(grad), ptr(d), d.stride(1) if d is not None else 0, stream_handle()), "ce_loss")
    return out[0], out[1], d


def rmsnorm_bwd(x, w, dy, eps, want_dw=True, residual=None):
    """Autograd of LlamaRMSNorm: (dx, dw).  residual: the gradient arriving over the skip connection, added to dx in the same pass (dx = residual + dx_norm)."""
    _need_cuda(x, w, dy, residual)
    rows, H = x.shape
    dx = torch.empty_like(x)
    dw = torch.empty(H, dtype=torch.float32, device=x.device) if want_dw else None
    inv = torch.empty((rows + 63) // 64 * 64 + (rows + 127) // 128 * H, dtype=torch.float32, device=x.device)   # inverse norms + the dw partial rows
    if residual is None:
        check(lib.lmx_op_rmsnorm_bwd(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(dy), ptr(dx), ptr(dw), ptr(inv), rows, H, eps, stream_handle()), "rmsnorm_bwd")
    else:
        assert residual.shape == x.shape and residual.dtype == x.dtype
        check(lib.lmx_op_rmsnorm_bwd_add(torch_dtype_code(x.dtype), ptr(x), ptr(w), ptr(dy), ptr(residual), ptr(dx), ptr(dw), ptr(inv), rows, H, eps, stream_handle()),
              "rmsnorm_bwd_add")
    return dx, dw


def swiglu_bwd(gate, up, dact):
    _need_cuda(gate, up, dact)
    dg, du = torch.empty_like(gate), torch.empty_like(up)
    check(lib.lmx_op_swiglu_bwd(torch_dtype_code(gate.dtype), ptr(gate), ptr(up), ptr(dact), ptr(dg), ptr(du), gate.numel(), stream_handle()), "swiglu_bwd")
    return dg, du


def rope_bwd(dy, cos_sin, pos0, heads, head_dim):
    """dy [T, heads*head_dim] (gradient w.r.t. the ROTATED q or k) -> gradient w.r.t. the un-rotated one."""
    _need_cuda(dy, cos_sin)
    dx = torch.empty_like(dy)
    check(lib.lmx_op_rope_bwd(torch_dtype_code(dy.dtype), ptr(dy), ptr(dx), ptr(cos_sin), pos0, dy.shape[0], heads, head_dim, dy.stride(0), stream_handle()), "rope_bwd")
    return dx


def transpose(x):
    _need_cuda(x)
    r, c = x.shape
    out = torch.empty((c, r), dtype=x.dtype, device=x.device)
    check(lib.lmx_op_transpose(torch_dtype_code(x.dtype), ptr(x), x.stride(0), r, c, ptr(out), out.stride(0), stream_handle()), "transpose")
    return out


def linear_bwd(x, w, dy):
    """Gradients of y = x @ w.T on the forward GEMM kernels: dx = dy @ w (contract over N: w transposed once), dw = dy.T @ x (contract over M)."""
    dx = gemm(dy, transpose(w))
    dw = gemm(transpose(dy), transpose(x))
    return dx, dw


def attn_bwd(q, k, v, d_out, heads, kv_heads, head_dim):
    """Causal attention backward.  q, d_out: [T, heads*D]; k, v: [T, kv_heads*D] (k, q already rotated) -> dq, dk, dv."""
    _need_cuda(q, k, v, d_out)
    T = q.shape[0]
    dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
    s1 = torch.empty(T * kv_heads * head_dim, dtype=torch.float32, device=q.device); s2 = torch.empty_like(s1)
    check(lib.lmx_op_attn_bwd(torch_dtype_code(q.dtype), head_dim, ptr(q), ptr(k), ptr(v), ptr(d_out), ptr(dq), ptr(s1), ptr(s2), ptr(dk), ptr(dv), T, heads,
                              kv_heads, q.stride(0), k.stride(0), d_out.stride(0), 1.0 / math.sqrt(head_dim), stream_handle()), "attn_bwd")
    return dq, dk, dv


def attn_bwd_lse(q, k, v, out, d_out, lse, heads, kv_heads, head_dim):
    """attn_bwd with the forward's output and log-sum-exp (flash_attn(..., lse=...)) as inputs: no statistics sweep in the backward (16-bit dtypes)."""
    _need_cuda(q, k, v, out, d_out, lse)
    T = q.shape[0]
    dq = torch.empty_like(q); dk = torch.empty_like(k); dv = torch.empty_like(v)
    check(lib.lmx_op_attn_bwd_lse(torch_dtype_code(q.dtype), head_dim, ptr(q), ptr(k), ptr(v), ptr(out), ptr(d_out), ptr(lse), lse.stride(0), ptr(dq), ptr(dk), ptr(dv),
                                  T, heads, kv_heads, q.stride(0), k.stride(0), d_out.stride(0), out.stride(0), 1.0 / math.sqrt(head_dim), stream_handle()), "attn_bwd_lse")
    return dq, dk, dv


# ---- pieces of one optimisation step (csrc/train.hip, composed by llava_mi355x/train.py) ----------------------------------------------
EW_SWIGLU, EW_GELU, EW_GELU_BWD, EW_ADD = 0, 1, 2, 3


def elementwise(op, a, b=None, out=None):
    """op 0: silu(a) * b (HF rounding points); 1: gelu_erf(a); 2: b * gelu'(a); 3: a + b.  Contiguous tensors of one shape."""
    _need_cuda(a, b)
    assert a.is_contiguous() and (b is None or (b.is_contiguous() and b.shape == a.shape))
    if out is None:
        out = torch.empty_like(a)
    check(lib.lmx_op_elementwise(torch_dtype_code(a.dtype), int(op), ptr(a), ptr(b), ptr(out), a.numel(), stream_handle()), "elementwise")
    return out


def cast_f32(src, out, accumulate=False):
    """fp32 accumulator -> `out` (parameter dtype), same number of elements.  accumulate: out = T(fp32(out) + src), one rounding (gradient accumulation)."""
    _need_cuda(src, out)
    assert src.dtype == torch.float32 and src.numel() == out.numel() and src.is_contiguous() and out.is_contiguous()
    fn = lib.lmx_op_cast_f32_add if accumulate else lib.lmx_op_cast_f32
    check(fn(torch_dtype_code(out.dtype), ptr(src), ptr(out), src.numel(), stream_handle()), "cast_f32_add" if accumulate else "cast_f32")
    return out


def col_sum(dy, out=None):
    """fp32 column sums of dy [rows, cols] (bias gradient); dy may be a column window of a wider buffer."""
    _need_cuda_rows(dy)
    _need_cuda(out)
    if out is None:
        out = torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device)
    assert out.dtype == torch.float32 and out.numel() == dy.shape[1]
    check(lib.lmx_op_col_sum(torch_dtype_code(dy.dtype), ptr(dy), dy.stride(0), dy.shape[0], dy.shape[1], ptr(out), stream_handle()), "col_sum")
    return out


def gather_embed(src, table, feats=None, out=None):
    """Rows of `table` (src >= 0), zero rows (src == -1) and rows of `feats` (src == -2 - k) -> [len(src), H] (into `out` when given)."""
    _need_cuda(src, table, feats, out)
    assert src.dtype == torch.int32 and table.is_contiguous() and (feats is None or feats.is_contiguous())
    if out is None:
        out = torch.empty((src.numel(), table.shape[1]), dtype=table.dtype, device=table.device)
    assert out.shape == (src.numel(), table.shape[1]) and out.dtype == table.dtype
    check(lib.lmx_op_gather_embed(torch_dtype_code(table.dtype), ptr(src), ptr(table), ptr(feats), ptr(out), src.numel(), table.shape[1], stream_handle()),
          "gather_embed")
    return out


def embed_bwd(src, d_embeds, dtable32=None, dfeats=None):
    """Autograd of gather_embed: token rows add into dtable32 (fp32 [V, H], caller zeroes it), feature rows are copied into dfeats."""
    _need_cuda(src, d_embeds, dtable32, dfeats)
    assert d_embeds.is_contiguous()
    check(lib.lmx_op_embed_bwd(torch_dtype_code(d_embeds.dtype), ptr(src), ptr(d_embeds), ptr(dtable32), ptr(dfeats), src.numel(), d_embeds.shape[1],
                               stream_handle()), "embed_bwd")


def sumsq(x, acc):
    """acc[0] += sum(x^2) (fp32 device scalar)."""
    _need_cuda(x, acc)
    assert x.is_contiguous() and acc.dtype == torch.float32
    check(lib.lmx_op_sumsq(torch_dtype_code(x.dtype), ptr(x), x.numel(), ptr(acc), stream_handle()), "sumsq")


def adamw(param, grad, master, exp_avg, exp_avg_sq, lr, betas, eps, weight_decay, step, gnorm_sq=None, max_grad_norm=0.0):
    """One torch.optim.AdamW update on fp32 master weights; `param` receives the rounded copy.  gnorm_sq: device fp32 scalar holding the
    squared global gradient norm (clip factor min(1, max_grad_norm / (norm + 1e-6)) is applied on the device)."""
    _need_cuda(param, grad, master, exp_avg, exp_avg_sq, gnorm_sq)
    n = param.numel()
    assert grad.numel() == n and master.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n and grad.dtype == param.dtype
    check(lib.lmx_op_adamw(torch_dtype_code(param.dtype), ptr(param), ptr(grad), ptr(master), ptr(exp_avg), ptr(exp_avg_sq), n, float(lr), float(betas[0]),
                           float(betas[1]), float(eps), float(weight_decay), int(step), ptr(gnorm_sq), float(max_grad_norm), stream_handle()), "adamw")


def wgrad_direct_ok(dy, x, out):
    """True if lmx_op_gemm_wgrad takes this call (16-bit, out / in features multiples of 256, rows a multiple of 64, aligned): no transposed copies needed."""
    if dy.dtype == torch.float32 or dy.dtype != x.dtype or out.dtype != dy.dtype or dy.stride(1) != 1 or x.stride(1) != 1 or out.stride(1) != 1:
        return False
    if (dy.data_ptr() | x.data_ptr() | out.data_ptr()) & 15:
        return False
    return bool(lib.lmx_op_gemm_wgrad_supported(torch_dtype_code(dy.dtype), dy.stride(0), x.stride(0), dy.shape[0], dy.shape[1], x.shape[1], out.stride(0)))


def gemm_wgrad(dy, x, out, accumulate=False):
    """out [O, I] = dy[R, O]^T @ x[R, I] with both operands in their forward layout (csrc/gemm8t.hip); fails loudly on shapes wgrad_direct_ok rejects.
    accumulate: out = T(fp32(out) + the product), the prior added to the fp32 sum before the one rounding (gradient accumulation)."""
    _need_cuda_rows(dy, x, out)
    assert dy.shape[0] == x.shape[0] and tuple(out.shape) == (dy.shape[1], x.shape[1])
    fn = lib.lmx_op_gemm_wgrad_acc if accumulate else lib.lmx_op_gemm_wgrad
    check(fn(torch_dtype_code(dy.dtype), ptr(dy), dy.stride(0), ptr(x), x.stride(0), dy.shape[0], dy.shape[1], x.shape[1], ptr(out), out.stride(0), stream_handle()),
          "gemm_wgrad_acc" if accumulate else "gemm_wgrad")
    return out


def lora_wgrad_ok(big, small, out, r_out=None, transposed=False):
    """True if lmx_op_lora_wgrad takes this call (16-bit, rows and big's columns multiples of 64, small 64 / 128 / 192 / 256 columns wide, aligned)."""
    if big.dtype == torch.float32 or big.dtype != small.dtype or out.dtype != big.dtype or big.stride(1) != 1 or small.stride(1) != 1 or out.stride(1) != 1:
        return False
    if big.shape[0] != small.shape[0] or (big.data_ptr() | small.data_ptr()) & 15:
        return False
    r_out = small.shape[1] if r_out is None else r_out
    return bool(lib.lmx_op_lora_wgrad_supported(torch_dtype_code(big.dtype), big.stride(0), small.stride(0), big.shape[0], big.shape[1], small.shape[1], r_out,
                                                int(transposed), out.stride(0)))


def lora_wgrad(big, small, out=None, alpha=1.0, r_out=None, transposed=False, n_slices=0, accumulate=False):
    """out = alpha * big[rows, F]^T @ small[rows, R][:, :r_out], stored [F, r_out] or, transposed, [r_out, F]; both operands in their forward layout
    (csrc/lora.hip).  The gradient of a LoRA factor: (dy, u) -> dB, (x, du) transposed -> dA.  Fails loudly on shapes lora_wgrad_ok rejects.
    accumulate: out = T(alpha * product + fp32(out)), one rounding (gradient accumulation: `out` holds the prior)."""
    _need_cuda_rows(big, small, out)
    rows, F = big.shape
    R = small.shape[1]
    r_out = R if r_out is None else r_out
    shape = (r_out, F) if transposed else (F, r_out)
    if out is None:
        out = torch.empty(shape, dtype=big.dtype, device=big.device)
    assert small.shape[0] == rows and tuple(out.shape) == shape and out.dtype == big.dtype == small.dtype
    nbytes = int(lib.lmx_op_lora_wgrad_workspace(rows, F, R, n_slices))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=big.device)
    fn = lib.lmx_op_lora_wgrad_acc if accumulate else lib.lmx_op_lora_wgrad
    check(fn(torch_dtype_code(big.dtype), ptr(big), big.stride(0), ptr(small), small.stride(0), rows, F, R, r_out, float(alpha), int(transposed),
             int(n_slices), ptr(out), out.stride(0), ptr(ws), nbytes, stream_handle()), "lora_wgrad_acc" if accumulate else "lora_wgrad")
    return out


def _drop_args(p, seed, step, stream):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1) (got {p})")
    return p, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF


def dropout_ok(x, out=None):
    """True if lmx_op_dropout / lmx_op_dropout_add take these operands (2-D, contiguous rows, columns and row strides multiples of 8, 16-byte aligned)."""
    out = x if out is None else out
    if x.dim() != 2 or out.dim() != 2 or x.stride(1) != 1 or out.stride(1) != 1 or x.dtype != out.dtype or x.shape != out.shape or (x.data_ptr() | out.data_ptr()) & 15:
        return False
    if x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        return False
    return bool(lib.lmx_op_dropout_supported(torch_dtype_code(x.dtype), x.stride(0), out.stride(0), x.shape[0], x.shape[1]))


def dropout(x, p, seed, step, stream, out=None):
    """The LoRA dropout of x [rows, cols] (csrc/dropout.h, dropout.py): kept elements T(x * fp32(1 / (1 - p))), dropped ones +0, the mask a function of
    (seed, row, column, stream, step).  The materialising form: the fp32 verification step, shapes the fused kernels refuse, and their yardstick.  out may be x."""
    _need_cuda_rows(x, out)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    assert out.shape == x.shape and out.dtype == x.dtype
    p, seed, step, stream = _drop_args(p, seed, step, stream)
    check(lib.lmx_op_dropout(torch_dtype_code(x.dtype), ptr(x), x.stride(0), ptr(out), out.stride(0), x.shape[0], x.shape[1], p, seed, step, stream, stream_handle()),
          "dropout")
    return out


def dropout_add(into, t, p, seed, step, stream):
    """into <- T(into + mask * scale * t), the sum in fp32: the adapter's share of dx, with the mask of the adapter's input on t = du A."""
    _need_cuda_rows(into, t)
    assert into.shape == t.shape and into.dtype == t.dtype
    p, seed, step, stream = _drop_args(p, seed, step, stream)
    check(lib.lmx_op_dropout_add(torch_dtype_code(t.dtype), ptr(into), into.stride(0), ptr(t), t.stride(0), t.shape[0], t.shape[1], p, seed, step, stream,
                                 stream_handle()), "dropout_add")
    return into


def lora_down_dropout_ok(x, A_stack, G, out=None):
    """True if lmx_op_lora_down_dropout takes this call (16-bit, rows and K multiples of 64, Rp = A_stack rows / G in {64, 128, 192, 256}, G <= 3, aligned)."""
    if x.dim() != 2 or A_stack.dim() != 2 or x.dtype == torch.float32 or x.dtype != A_stack.dtype or x.stride(1) != 1 or A_stack.stride(1) != 1:
        return False
    if G < 1 or A_stack.shape[0] % G or A_stack.shape[1] != x.shape[1] or (x.data_ptr() | A_stack.data_ptr()) & 15:
        return False
    if out is not None and (out.dtype != x.dtype or out.stride(1) != 1 or tuple(out.shape) != (x.shape[0], A_stack.shape[0]) or out.data_ptr() & 15):
        return False
    ldu = A_stack.shape[0] if out is None else out.stride(0)
    return bool(lib.lmx_op_lora_down_dropout_supported(torch_dtype_code(x.dtype), x.stride(0), A_stack.stride(0), ldu, x.shape[0], x.shape[1], A_stack.shape[0] // G, G))


def lora_down_dropout(x, A_stack, G, p, seed, step, stream0, out=None):
    """u [rows, G Rp] with u[:, g Rp:(g + 1) Rp] = dropout_g(x) @ A_g^T for the G adapters that share the input x (A_stack [G Rp, K]; adapter g masks with stream
    stream0 + g).  The mask is applied inside the kernel (csrc/lora.hip): no masked copy of x is written.  Fails loudly on shapes lora_down_dropout_ok rejects."""
    _need_cuda_rows(x, A_stack, out)
    rows, K = x.shape
    if out is None:
        out = torch.empty((rows, A_stack.shape[0]), dtype=x.dtype, device=x.device)
    assert A_stack.shape[0] % G == 0 and A_stack.shape[1] == K and tuple(out.shape) == (rows, A_stack.shape[0]) and out.dtype == x.dtype == A_stack.dtype
    p, seed, step, stream0 = _drop_args(p, seed, step, stream0)
    check(lib.lmx_op_lora_down_dropout(torch_dtype_code(x.dtype), ptr(x), x.stride(0), ptr(A_stack), A_stack.stride(0), ptr(out), out.stride(0), rows, K,
                                       A_stack.shape[0] // G, int(G), p, seed, step, stream0, stream_handle()), "lora_down_dropout")
    return out


def lora_wgrad_dropout(big, small, p, seed, step, stream, out=None, alpha=1.0, r_out=None, transposed=False, n_slices=0, accumulate=False):
    """lora_wgrad with the LoRA dropout mask applied to `big` inside the kernel: dA = du^T dropout(x) for (x, du), transposed.  Takes what lora_wgrad_ok takes.
    accumulate: as lora_wgrad."""
    _need_cuda_rows(big, small, out)
    rows, F = big.shape
    R = small.shape[1]
    r_out = R if r_out is None else r_out
    shape = (r_out, F) if transposed else (F, r_out)
    if out is None:
        out = torch.empty(shape, dtype=big.dtype, device=big.device)
    assert small.shape[0] == rows and tuple(out.shape) == shape and out.dtype == big.dtype == small.dtype
    p, seed, step, stream = _drop_args(p, seed, step, stream)
    nbytes = int(lib.lmx_op_lora_wgrad_workspace(rows, F, R, n_slices))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=big.device)
    fn = lib.lmx_op_lora_wgrad_dropout_acc if accumulate else lib.lmx_op_lora_wgrad_dropout
    check(fn(torch_dtype_code(big.dtype), ptr(big), big.stride(0), ptr(small), small.stride(0), rows, F, R, r_out, float(alpha), int(transposed), int(n_slices),
             ptr(out), out.stride(0), ptr(ws), nbytes, p, seed, step, stream, stream_handle()), "lora_wgrad_dropout_acc" if accumulate else "lora_wgrad_dropout")
    return out


def transpose_padded(x, multiple):
    """x [r, c] -> [c, roundup(r, multiple)] with zero columns past r: the operand layout of a GEMM that contracts over r."""
    _need_cuda_rows(x)
    r, c = x.shape
    rp = -(-r // multiple) * multiple
    out = torch.empty((c, rp), dtype=x.dtype, device=x.device) if rp == r else torch.zeros((c, rp), dtype=x.dtype, device=x.device)
    check(lib.lmx_op_transpose(torch_dtype_code(x.dtype), ptr(x), x.stride(0), r, c, ptr(out), out.stride(0), stream_handle()), "transpose")
    return out
