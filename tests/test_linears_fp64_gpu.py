"""The decode GEMV family (gemv_kernel in csrc/gemm.hip, gemv2_body in csrc/gemv2.h) and the ring / LDS-DMA GEMM variants + the fp32 GEMM (csrc/gemm.hip) against
float64, element by element, through the C ABI.

References and bounds: tests/linear_ref.py.  The GEMV bound is derived there from the kernels' arithmetic (fp32 fmaf chain of 8 ceil(K / 512) terms per lane, six
levels of wave_sum, fp32 epilogue, ONE rounding to the storage dtype) and is never tuned on the device; the 16-bit GEMMs are held to one ulp of the once-rounded
float64 result with the project's accumulation-noise constants of test_gemm8p_gpu.py.

x and the norm weights of every GEMV case are drawn on the HOST from a per-case seed, so the only input-dependent condition of the bound — the share of x elements
whose first rounding the kernel's fp32 `inv` can move (at most 1 % of K) — can be checked without a device; it is asserted in every test that relies on it."""
import math
import zlib

import pytest
import torch

import linear_ref as L

pytestmark = pytest.mark.gpu

DT = L.DT
NONE, QGELU, GELU, SILU = L.ACT_NONE, L.ACT_QUICK_GELU, L.ACT_GELU_ERF, L.ACT_SILU_MUL


# ---- which kernel a single 16-bit row takes: launch_gemv2's rules (csrc/gemm.hip), restated ------------------------------------------------------------------------
def gemv2_config(N, K, norm, silu):
    """(R, P, NX) of the gemv2_body instantiation lmx_op_gemv launches for one 16-bit row, or None where gemv2_applies() declines (K > 16384) and
    gemv_kernel<T, 1, R> runs instead."""
    if K > 16384:
        return None
    NX = 2 if K <= 4096 else 4 if K <= 8192 else 6 if K <= 12288 else 8
    if silu:
        return (2, 4, NX)
    if K >= 8192:
        return (1, 8, NX)
    if N * K <= 1 << 25:
        return (2, 4, NX) if norm else (1, 2, NX)
    return (2, 4, NX)


# every (R, P, NX) that launch_gemv2 can reach: (1, 8) needs K >= 8192, i.e. NX >= 4; (1, 2) needs K < 8192, i.e. NX <= 4.  (1, 8, 2), (1, 2, 6) and (1, 2, 8) are
# instantiated by the template dispatch but no shape selects them.
REACHABLE = {(1, 2, 2), (1, 2, 4), (1, 8, 4), (1, 8, 6), (1, 8, 8), (2, 4, 2), (2, 4, 4), (2, 4, 6), (2, 4, 8)}


def _case(name, N, K, norm=False, res=False, silu=False, bias=False, act=NONE, scale=1.0):
    cfg = gemv2_config(N, K, norm, silu)
    tag = "gemv_kernel" if cfg is None else "R%dP%dNX%d" % cfg
    return pytest.param(dict(name=name, N=N, K=K, norm=norm, res=res, act=SILU if silu else act, bias=bias, scale=scale, cfg=cfg), id=f"{name}-{N}x{K}-{tag}")


GEMV2_CASES = [
    # LLaVA-1.5-7B decode step, each with the prologue / epilogue the engine fuses into it
    _case("qkv7b", 12288, 4096, norm=True), _case("q7b", 4096, 4096, norm=True), _case("o7b", 4096, 4096, res=True),
    _case("gateup7b", 22016, 4096, norm=True, silu=True), _case("down7b", 4096, 11008, res=True), _case("lmhead", 32000, 4096, norm=True),
    # 13B
    _case("qkv13b", 15360, 5120, norm=True), _case("gateup13b", 27648, 5120, norm=True, silu=True), _case("down13b", 5120, 13824, res=True),
    # tensor-parallel rank shapes (2 / 4 / 8 ranks): o_proj and down_proj read a K slice and add the residual, lm_head writes a shard
    _case("o_tp2", 4096, 2048, res=True), _case("o_tp4", 4096, 1024, res=True), _case("o_tp8", 4096, 512, res=True),
    _case("down_tp2", 4096, 5504, res=True), _case("down_tp4", 4096, 2752, res=True), _case("down_tp8", 4096, 1376, res=True),
    _case("down13b_tp2", 5120, 6912, res=True), _case("down13b_tp4", 5120, 3456, res=True), _case("down13b_tp8", 5120, 1728, res=True),
    _case("lmhead_tp2", 16000, 4096, norm=True),
    # the remaining instantiations
    _case("k8192", 1024, 8192, res=True), _case("silu_k8192", 256, 8192, norm=True, silu=True), _case("silu_k11008", 512, 11008, silu=True),
    _case("silu_k16384", 128, 16384, norm=True, silu=True),
    # K edges: one chunk; KC = 63 (a partial only round); KC = 65 (one lane in round 2); fewer rounds than the ring is deep (NR = 1 < P = 4); rounds no multiple of P
    # (K = 5504: NR = 11, P = 2; K = 11008: NR = 22, P = 8); the last K gemv2_applies accepts and the first it declines
    _case("k8", 64, 8, res=True), _case("k8_norm", 64, 8, norm=True), _case("k504", 200, 504, res=True), _case("k520", 200, 520, norm=True),
    _case("k512_p4", 264, 512, norm=True), _case("k16384", 264, 16384, res=True), _case("k16392", 264, 16392, res=True), _case("k16392_norm", 72, 16392, norm=True),
    # N edges: one output; one short of / one past a workgroup's 4 R rows, for R = 1 (no norm) and R = 2 (norm)
    _case("n1_r1", 1, 1024, res=True), _case("n3_r1", 3, 1024, res=True), _case("n5_r1", 5, 1024, bias=True),
    _case("n1_r2", 1, 1024, norm=True), _case("n7_r2", 7, 1024, norm=True), _case("n9_r2", 9, 1024, norm=True, res=True),
    # SiLU*mul with a half-empty last workgroup (N / 2 = 32, 96: 16 outputs per workgroup of 4 waves x 2 rows... 8 pairs), with a bias
    _case("silu_i32", 64, 1024, norm=True, silu=True), _case("silu_i96", 192, 1024, norm=True, silu=True, bias=True),
    # bias + activation in the single-row kernels (the CLIP-style epilogues), pre-activations down to -6
    _case("bias_qgelu", 1000, 1024, bias=True, act=QGELU, res=True), _case("bias_gelu", 1000, 1024, bias=True, act=GELU, res=True),
    _case("norm_bias_gelu", 1000, 4096, norm=True, bias=True, act=GELU),
    # inv far from 1: x scaled by 64 and by 1 / 64
    _case("q7b_x64", 4096, 4096, norm=True, scale=64.0), _case("q7b_x1_64", 4096, 4096, norm=True, scale=1 / 64),
    _case("silu_x64", 192, 1024, norm=True, silu=True, scale=64.0), _case("silu_x1_64", 192, 1024, norm=True, silu=True, scale=1 / 64),
    _case("k16392_x64", 72, 16392, norm=True, scale=64.0), _case("k16392_x1_64", 72, 16392, norm=True, scale=1 / 64),
]


SALT = 0          # part of every seed; chosen on the host so that every case's flippable set stays under the cap (test_linears_fp64_cases.py re-checks it)


def _seed(*key):
    return zlib.crc32(repr((SALT,) + key).encode())


def _host_inputs(MB, K, dt, norm, scale, seed):
    """x [MB, K] ~ N(0, 1) * scale and the RMSNorm weight 1 + 0.1 N(0, 1), drawn on the host (see the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(MB, K, generator=g) * scale).to(DT[dt])
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(DT[dt]) if norm else None
    return x, nw


def _make(c, dt, cuda, MB=1):
    """Inputs of one case on the device: (x, w for the kernel, w for the reference, bias, bias for the reference, residual, norm_w)."""
    from llava_mi355x import ops
    N, K, act = c["N"], c["K"], c["act"]
    seed = _seed(c["name"], N, K, dt, MB)
    x, nw = _host_inputs(MB, K, dt, c["norm"], c["scale"], seed)
    x = x.to(cuda); nw = nw.to(cuda) if nw is not None else None
    g = torch.Generator(device=cuda).manual_seed(seed + 1)
    T = DT[dt]
    w = (torch.randn(N, K, device=cuda, generator=g) / math.sqrt(K)).to(T)
    # pre-activations down to -6 where an activation follows: a bias of 3 N(0, 1) on top of the N(0, 1) product
    b = ((3.0 if act in (QGELU, GELU) else 1.0) * torch.randn(N, device=cuda, generator=g)).to(T) if c["bias"] else None
    n_out = N // 2 if act == SILU else N
    r = torch.randn(MB, n_out, device=cuda, generator=g).to(T) if c["res"] else None
    if act == SILU:
        I = N // 2
        w_ref = (w[:I], w[I:]); b_ref = (b[:I], b[I:]) if b is not None else None
        w_k = ops.interleave_gate_up(w[:I].contiguous(), w[I:].contiguous())
        b_k = torch.cat([b[:I].view(I // 32, 32), b[I:].view(I // 32, 32)], 1).reshape(N).contiguous() if b is not None else None
    else:
        w_ref, b_ref, w_k, b_k = w, b, w, b
    return x, w_k, w_ref, b_k, b_ref, r, nw


def _flips_ok(frac, K, what):
    assert frac <= L.FLIP_MAX_FRACTION, f"{what}: {frac:.4f} of the {K} x elements sit on a rounding boundary of the norm prologue (cap {L.FLIP_MAX_FRACTION})"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c", GEMV2_CASES)
def test_gemv_single_row_vs_fp64(cuda, dt, c):
    """Every gemv2_body instantiation (and gemv_kernel<T, 1, R> past K = 16384) within ulp_T(ref) + the derived fp32 bound of the float64 statement, per output."""
    from llava_mi355x import ops
    x, w_k, w_ref, b_k, b_ref, r, nw = _make(c, dt, cuda)
    got = ops.gemv(x, w_k, bias=b_k, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
    ref, E, frac = L.linear_ref(x, w_ref, dt, bias=b_ref, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
    _flips_ok(frac, c["K"], c["name"])
    worst = L.check(got, ref, E, dt, f"{c['name']} {dt}")
    print(f"GEMV1 {c['name']} {dt} cfg={c['cfg']} worst_err_over_bound={worst:.3f} flip_fraction={frac:.5f}")
    if r is not None:                         # in place on the residual stream, as the engine runs o_proj and down_proj
        r2 = r.clone()
        ops.gemv(x, w_k, bias=b_k, residual=r2, norm_w=nw, eps=1e-5, act=c["act"], out=r2)
        assert torch.equal(r2, got), "out aliasing the residual changed the result"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c", GEMV2_CASES)
def test_gemv2_bits_equal_gemv_kernel(cuda, dt, c):
    """gemv2.h's claim: the hand-counted stream computes the bits of gemv_kernel<T, 1, R>.  One row through lmx_op_gemv (gemv2_body) against the same row twice
    through the two-row launch (gemv_kernel<T, 2, R>: compiler-scheduled loads, the same staging, per-lane order, reduction and epilogue)."""
    from llava_mi355x import ops
    x, w_k, _, b_k, _, r, nw = _make(c, dt, cuda)
    one = ops.gemv(x, w_k, bias=b_k, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
    two = ops.gemv(torch.cat([x, x]), w_k, bias=b_k, residual=torch.cat([r, r]) if r is not None else None, norm_w=nw, eps=1e-5, act=c["act"])
    for row in (0, 1):
        ne = one[0] != two[row]
        assert not bool(ne.any()), (f"{c['name']} {dt}: {int(ne.sum())} of {ne.numel()} outputs differ between the one-row and the two-row kernel (row {row}); "
                                    f"max |diff| {float((one[0].float() - two[row].float()).abs().max()):.3e}")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("c", [p for p in GEMV2_CASES if p.values[0]["name"] in ("qkv7b", "o7b", "gateup7b", "down7b", "lmhead", "qkv13b", "gateup13b", "down13b")])
def test_gemv2_launch_to_launch_bits_under_uneven_load(cuda, dt, c):
    """20 launches of each real decode shape alternating two inputs while an unrelated matmul shares the chip every third launch: each launch reproduces the bits of
    the first launch on its input.  A wait count one round short in the hand-counted stream shows as run-to-run difference, not as a large error."""
    from llava_mi355x import ops
    xa, w_k, _, b_k, _, r, nw = _make(c, dt, cuda)
    xb = torch.flip(xa, dims=(1,)).contiguous()
    side = torch.cuda.Stream()
    junk = torch.randn(4096, 4096, device=cuda)
    first = [None, None]
    for it in range(20):
        i = it & 1
        if it % 3 == 0:
            with torch.cuda.stream(side):
                junk @ junk
        got = ops.gemv((xa, xb)[i], w_k, bias=b_k, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
        if first[i] is None:
            first[i] = got.clone()
        else:
            assert torch.equal(got, first[i]), f"launch {it}: not the bits of the first launch on input {i}"
    torch.cuda.synchronize()


# ---- gemv_kernel: 1..4 rows, every storage dtype, R = 1 / 2 / 4 ----------------------------------------------------------------------------------------------------
# launch_gemv_mb: R = 1 up to 2^24 weights, above that 2 (N < 8192) or 4; SiLU*mul always 2.  N is no multiple of 4 R so the last workgroup has clamped dummy rows;
# K = 4104 / 2056 leave a partial last round (KC % 64 != 0).  The SiLU*mul mode takes N rounded down to a multiple of 64.
MB_SHAPES = [pytest.param(264 + 2, 512, 1, id="R1-266x512"), pytest.param(4100 + 2, 4104, 2, id="R2-4102x4104"), pytest.param(8200 + 2, 2056, 4, id="R4-8202x2056")]
MODES = {"plain": dict(), "bias": dict(bias=True), "bias_qgelu": dict(bias=True, act=QGELU), "bias_gelu_res": dict(bias=True, act=GELU, res=True),
         "norm": dict(norm=True), "norm_silu": dict(norm=True, silu=True), "res_inplace": dict(res=True)}


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("MB", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K,R", MB_SHAPES)
def test_gemv_rows_vs_fp64(cuda, dt, mode, MB, N, K, R):
    from llava_mi355x import ops
    m = MODES[mode]
    if m.get("silu"):
        N = N // 64 * 64
    else:
        assert (N * K <= 1 << 24) == (R == 1) and (N >= 8192) == (R == 4), "the shape no longer selects the R it is named for"
    c = _case(f"rows_{mode}", N, K, **m).values[0]
    x, w_k, w_ref, b_k, b_ref, r, nw = _make(c, dt, cuda, MB)
    ref, E, frac = L.linear_ref(x, w_ref, dt, bias=b_ref, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
    _flips_ok(frac, K, mode)
    if mode == "res_inplace":
        out = r.clone()
        got = ops.gemv(x, w_k, residual=out, out=out)
    else:
        got = ops.gemv(x, w_k, bias=b_k, residual=r, norm_w=nw, eps=1e-5, act=c["act"])
    worst = L.check(got, ref, E, dt, f"{mode} MB={MB} {N}x{K} {dt}")
    print(f"GEMVMB {mode} MB={MB} {N}x{K} {dt} worst_err_over_bound={worst:.3f} flip_fraction={frac:.5f}")


def host_norm_inputs():
    """(label, dt, x) for every case above and below that runs the norm prologue: the host-drawn inputs the flippable-set cap is checked on."""
    for dt in ("bf16", "f16"):
        for p in GEMV2_CASES:
            c = p.values[0]
            if c["norm"]:
                yield c["name"], dt, _host_inputs(1, c["K"], dt, True, c["scale"], _seed(c["name"], c["N"], c["K"], dt, 1))[0]
        for MB in (1, 2, 3, 4):
            for sp in MB_SHAPES:
                N, K, _ = sp.values
                for mode, m in MODES.items():
                    if m.get("norm"):
                        NN = N // 64 * 64 if m.get("silu") else N
                        yield f"rows_{mode} MB={MB} K={K}", dt, _host_inputs(MB, K, dt, True, 1.0, _seed(f"rows_{mode}", NN, K, dt, MB))[0]
        for wp in WINDOWS:
            MB, N, K, m = wp.values
            if m.get("norm"):
                yield f"win MB={MB} K={K}", dt, _host_inputs(MB, K, dt, True, 1.0, _seed("win", N, K, dt, MB))[0]


def test_gemv_silu_mul_rejects_a_residual(cuda):
    """kernels.h: the residual is added after the activation; the SiLU*mul epilogue has no such add, and launch_gemv says so instead of dropping the operand."""
    from llava_mi355x import _C, ops
    x = torch.randn(1, 256, device=cuda).bfloat16(); w = torch.randn(128, 256, device=cuda).bfloat16(); r = torch.zeros(1, 64, device=cuda).bfloat16()
    with pytest.raises(_C.LmxError, match="SiLU"):
        ops.gemv(x, w, residual=r, act=SILU)


# ---- strides and windows ---------------------------------------------------------------------------------------------------------------------------------------------
def _window(MB, N, K, **m):
    """One window case, named by the kernel a 16-bit launch of it takes (the fp32 parametrisation of every row runs gemv_kernel)."""
    cfg = gemv2_config(N, K, m.get("norm", False), m.get("silu", False)) if MB == 1 else None
    tag = "gemv_kernel" if cfg is None else "gemv2_R%dP%dNX%d" % cfg
    return pytest.param(MB, N, K, m, id=f"{tag}-MB{MB}-{N}x{K}-" + "_".join(sorted(k for k, v in m.items() if v)))


WINDOWS = [_window(1, 4096, 2048, res=True), _window(1, 1000, 4096, norm=True, res=True), _window(1, 1024, 11008, res=True), _window(1, 192, 1024, norm=True, silu=True),
           _window(1, 8000, 4096, norm=True), _window(3, 265, 520, bias=True, act=QGELU, res=True), _window(2, 4100, 4104, norm=True), _window(1, 72, 16392, res=True)]


@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("MB,N,K,m", WINDOWS)
def test_gemv_windows_of_wider_buffers(cuda, dt, MB, N, K, m):
    """x, w, residual and out as column windows of wider buffers (ldx != K, ldw != K, ldc != N, ldr != N — all of which the entry point takes and the engine uses):
    NaN around the inputs must not reach the result, and every byte of out's buffer outside [MB, N] stays as it was.  out starts an odd number of elements into its row,
    not 16-byte aligned — the lm_head shard written at a column offset of the full logits row."""
    from llava_mi355x import ops
    c = _case("win", N, K, **m).values[0]
    x0, w0, w_ref, b_k, b_ref, r0, nw = _make(c, dt, cuda, MB)
    T = DT[dt]
    nan = float("nan")
    xb = torch.full((MB + 1, K + 24), nan, dtype=T, device=cuda); x = xb[:MB, 8:8 + K]; x.copy_(x0)
    wb = torch.full((w0.shape[0] + 2, K + 16), nan, dtype=T, device=cuda); w = wb[1:1 + w0.shape[0], 8:8 + K]; w.copy_(w0)
    n_out = N // 2 if c["act"] == SILU else N
    r = None
    if r0 is not None:
        rb = torch.full((MB, n_out + 11), nan, dtype=T, device=cuda); r = rb[:, 5:5 + n_out]; r.copy_(r0)
    ob = torch.full((MB + 2, n_out + 13), 1234.0, dtype=T, device=cuda)
    before = ob.clone()
    c0 = next(c0 for c0 in (3, 5, 1) if ob[1:, c0:].data_ptr() % 16 != 0)
    out = ob[1:1 + MB, c0:c0 + n_out]
    assert x.stride(0) != K and w.stride(0) != K and out.stride(0) != n_out and out.data_ptr() % 16 != 0
    ops.gemv(x, w, bias=b_k, residual=r, norm_w=nw, eps=1e-5, act=c["act"], out=out)
    ref, E, frac = L.linear_ref(x0, w_ref, dt, bias=b_ref, residual=r0, norm_w=nw, eps=1e-5, act=c["act"])
    _flips_ok(frac, K, "window")
    L.check(out, ref, E, dt, f"windows MB={MB} {N}x{K} {dt}")
    assert torch.equal(out, ops.gemv(x0, w0, bias=b_k, residual=r0, norm_w=nw, eps=1e-5, act=c["act"])), "strided operands changed the bits"
    after = ob.clone(); after[1:1 + MB, c0:c0 + n_out] = before[1:1 + MB, c0:c0 + n_out]
    assert torch.equal(after.view(torch.uint8), before.view(torch.uint8)), "bytes outside out's [MB, N] window were written"


def test_gemv_rejects_misaligned_rows(cuda):
    """Every lane reads 16 bytes at a time: an x or weight window whose rows start off that grid is refused by launch_gemv, not read misaligned."""
    from llava_mi355x import _C, ops
    x = torch.randn(2, 64, device=cuda).bfloat16(); w = torch.randn(16, 64, device=cuda).bfloat16()
    wide = torch.randn(16, 72, device=cuda).bfloat16()
    with pytest.raises(_C.LmxError, match="16-byte"):
        ops.gemv(x, wide[:, 4:68])                               # rows start 8 bytes off
    with pytest.raises(_C.LmxError, match="16-byte"):
        ops.gemv(x, torch.randn(16, 68, device=cuda).bfloat16()[:, :64])      # row stride 136 bytes
    with pytest.raises(_C.LmxError, match="16-byte"):
        ops.gemv(wide[:2, 4:68], w)


# ---- ring / LDS-DMA GEMM variants -----------------------------------------------------------------------------------------------------------------------------------
RING = [2, 4, 5, 7, 9, 15, 16, 17, 18]
HAS_SILU = (2, 4, 7, 9, 18)              # the 64x64 tiles (5, 15, 16, 17) are rejected by "gemm: the 64x64 tile has no SiLU·mul epilogue"
# one K step (fewer steps than ring slots and than the K groups of 16 / 17), two, odd / even step counts, ragged M and N tails, one row, a long K
GEMM_SHAPES = [(128, 128, 64), (64, 64, 128), (1087, 512, 192), (577, 384, 640), (33, 136, 320), (300, 1024, 1024), (513, 776, 2048), (1, 8, 64), (257, 264, 4096)]


def _mk(M, N, K, dt, cuda, seed):
    g = torch.Generator(device=cuda).manual_seed(seed)
    x = torch.randn(M, K, device=cuda, generator=g).to(DT[dt])
    w = (torch.randn(N, K, device=cuda, generator=g) / math.sqrt(K)).to(DT[dt])
    return x, w, g


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("variant", RING)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_ring_gemm_plain_one_ulp(cuda, dt, variant, M, N, K):
    from llava_mi355x import ops
    x, w, _ = _mk(M, N, K, dt, cuda, _seed(M, N, K, variant))
    out = torch.full((M, N + 8), float("nan"), dtype=DT[dt], device=cuda)
    got = ops.gemm(x, w, variant=variant, out=out[:, :N])
    L.gemm16_check(got, x.double() @ w.double().t(), dt, False, f"variant {variant} {M}x{N}x{K} {dt}")
    assert torch.isnan(out[:, N:].float()).all(), "columns past N were written"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("act", [NONE, QGELU, GELU])
@pytest.mark.parametrize("variant", RING)
@pytest.mark.parametrize("M,N,K", [(300, 520, 320), (33, 136, 64)])
def test_ring_gemm_bias_act_residual(cuda, dt, act, variant, M, N, K):
    """bias + activation + residual in every ring variant (pre-activations down to -6), into a NaN-filled out with ldc > N, and with out aliasing the residual:
    the same bits."""
    from llava_mi355x import ops
    x, w, g = _mk(M, N, K, dt, cuda, _seed(M, N, K, variant, act))
    T = DT[dt]
    b = (3.0 * torch.randn(N, device=cuda, generator=g)).to(T); r = torch.randn(M, N, device=cuda, generator=g).to(T)
    y = x.double() @ w.double().t() + b.double()
    ref = L.act64(y, act)[0] + r.double()
    if act != NONE:
        assert float(y.min()) < -6.0
    out = torch.full((M, N + 12), float("nan"), dtype=T, device=cuda)
    got = ops.gemm(x, w, bias=b, residual=r, act=act, variant=variant, out=out[:, :N])
    L.gemm16_check(got, ref, dt, act != NONE, f"variant {variant} act {act} {dt}")
    assert torch.isnan(out[:, N:].float()).all(), "columns past N were written"
    r2 = r.clone()
    ops.gemm(x, w, bias=b, residual=r2, act=act, variant=variant, out=r2)
    assert torch.equal(r2, got), "out aliasing the residual changed the result"


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("variant", HAS_SILU)
@pytest.mark.parametrize("M,I,K", [(300, 352, 320), (33, 96, 64), (1, 32, 128)])
def test_ring_gemm_silu_mul(cuda, dt, variant, M, I, K):
    from llava_mi355x import ops
    x, w, _ = _mk(M, 2 * I, K, dt, cuda, _seed(M, I, K, variant))
    wg, wu = w[:I].contiguous(), w[I:].contiguous()
    ref = L.act64(x.double() @ wg.double().t(), SILU)[0] * (x.double() @ wu.double().t())
    out = torch.full((M, I + 8), float("nan"), dtype=DT[dt], device=cuda)
    got = ops.gemm(x, ops.interleave_gate_up(wg, wu), act=SILU, variant=variant, out=out[:, :I])
    L.gemm16_check(got, ref, dt, True, f"variant {variant} SiLU*mul {M}x{I}x{K} {dt}")
    assert torch.isnan(out[:, I:].float()).all(), "columns past N / 2 were written"


@pytest.mark.parametrize("variant", [5, 15, 16, 17])
def test_ring_gemm_64x64_tiles_reject_silu_mul(cuda, variant):
    from llava_mi355x import _C, ops
    x, w, _ = _mk(64, 128, 64, "bf16", cuda, 1)
    with pytest.raises(_C.LmxError, match="no SiLU"):
        ops.gemm(x, w, act=SILU, variant=variant)


# every 16-bit MFMA GEMM family: the ring / LDS-DMA variants, auto (0), the ping-pong kernel (30, 33) and the skinny decode-batch kernel (20, at most 32 rows)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("variant,M", [(v, 300) for v in RING + [0, 30, 33]] + [(20, 29)])
def test_gemm16_gelu_tail_is_relative(cuda, dt, variant, M):
    """bias + GELU-erf with pre-activations down to -6 and NO residual, so the output is the activation's own small value: held to linear_ref.gemm16_gelu_tail_check
    (relative where |ref| is small) next to the one-ulp check."""
    from llava_mi355x import ops
    N, K = 520, 320
    x, w, g = _mk(M, N, K, dt, cuda, _seed("tail", variant, M))
    b = (3.0 * torch.randn(N, device=cuda, generator=g)).to(DT[dt])
    y = x.double() @ w.double().t() + b.double()
    assert float(y.min()) < -6.0
    got = ops.gemm(x, w, bias=b, act=GELU, variant=variant)
    L.gemm16_check(got, L.act64(y, GELU)[0], dt, True, f"variant {variant} GELU {dt}")
    worst = L.gemm16_gelu_tail_check(got, y, dt, f"variant {variant} GELU tail {dt}")
    print(f"GELUTAIL variant={variant} {dt} worst_err_over_bound={worst:.3f}")


# the vision tower and the projector at their real shapes through variant 0 (whatever the launcher resolves it to): CLIP ViT-L/14-336 (577 tokens, width 1024, MLP
# 4096; the 14 x 14 x 3 = 588 patch pixels padded to K = 640) and the mlp2x_gelu projector (1024 -> 4096 -> 4096)
VISION = [("clip_qkv", 577, 3072, 1024, NONE, False), ("clip_out", 577, 1024, 1024, NONE, True), ("clip_fc1", 577, 4096, 1024, QGELU, False),
          ("clip_fc2", 577, 1024, 4096, NONE, True), ("patch_embed", 576, 1024, 640, None, False), ("proj_fc1", 576, 4096, 1024, GELU, False),
          ("proj_fc2", 576, 4096, 4096, NONE, False)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("images", [1, 2])
@pytest.mark.parametrize("name,M,N,K,act,inplace", VISION)
def test_vision_shape_gemm_one_ulp(cuda, dt, images, name, M, N, K, act, inplace):
    from llava_mi355x import ops
    M *= images
    x, w, g = _mk(M, N, K, dt, cuda, _seed(name, images))
    T = DT[dt]
    if name == "patch_embed":                                   # no bias; the pad columns of x are zero
        x[:, 588:] = 0
        got = ops.gemm(x, w, variant=0)
        L.gemm16_check(got, x.double() @ w.double().t(), dt, False, f"{name} {dt}")
        return
    b = torch.randn(N, device=cuda, generator=g).to(T)
    y = x.double() @ w.double().t() + b.double()
    ref = L.act64(y, act)[0]
    if inplace:                                                 # the residual stream: C aliases R
        r = torch.randn(M, N, device=cuda, generator=g).to(T)
        ref = ref + r.double()
        got = ops.gemm(x, w, bias=b, residual=r, act=act, variant=0, out=r)
    else:
        got = ops.gemm(x, w, bias=b, act=act, variant=0)
    L.gemm16_check(got, ref, dt, act != NONE, f"{name} x{images} {dt}")


# ---- the fp32 GEMM -----------------------------------------------------------------------------------------------------------------------------------------------------
# gemm_f32_kernel: no MFMA; each thread owns 4 x 4 outputs and adds the K products of one output in k order with fmaf into ONE accumulator (16 per LDS slab, slab
# after slab): a chain of K fused multiply-adds, no tree.  Bound: (K + epilogue) 2^-24 sum_k |x w| per element (linear_ref with chain = K, tree = 0).
@pytest.mark.parametrize("mode", ["plain", "bias_qgelu_res", "bias_gelu_res", "bias_res_inplace"])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32_vs_fp64(cuda, mode, M, N, K):
    from llava_mi355x import ops
    x, w, g = _mk(M, N, K, "f32", cuda, _seed(M, N, K, mode))
    b = r = None
    act = {"plain": NONE, "bias_qgelu_res": QGELU, "bias_gelu_res": GELU, "bias_res_inplace": NONE}[mode]
    if mode != "plain":
        b = 3.0 * torch.randn(N, device=cuda, generator=g); r = torch.randn(M, N, device=cuda, generator=g)
    ref, E, _ = L.linear_ref(x, w, "f32", bias=b, residual=r, act=act, chain=K, tree=0)
    if mode == "bias_res_inplace":
        got = r.clone(); ops.gemm(x, w, bias=b, residual=got, out=got)
    else:
        out = torch.full((M, N + 4), float("nan"), device=cuda)
        got = ops.gemm(x, w, bias=b, residual=r, act=act, out=out[:, :N])
        assert torch.isnan(out[:, N:]).all(), "columns past N were written"
    worst = L.check(got, ref, E, "f32", f"fp32 GEMM {mode} {M}x{N}x{K}")
    print(f"GEMMF32 {mode} {M}x{N}x{K} worst_err_over_bound={worst:.3f}")


@pytest.mark.parametrize("M,I,K", [(300, 352, 320), (33, 96, 64), (1, 32, 128)])
def test_gemm_f32_silu_mul_vs_fp64(cuda, M, I, K):
    from llava_mi355x import ops
    x, w, _ = _mk(M, 2 * I, K, "f32", cuda, _seed(M, I, K))
    wg, wu = w[:I].contiguous(), w[I:].contiguous()
    ref, E, _ = L.linear_ref(x, (wg, wu), "f32", act=SILU, chain=K, tree=0)
    got = ops.gemm(x, ops.interleave_gate_up(wg, wu), act=SILU)
    L.check(got, ref, E, "f32", f"fp32 GEMM SiLU*mul {M}x{I}x{K}")
