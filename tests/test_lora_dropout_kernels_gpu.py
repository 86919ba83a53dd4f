"""The four LoRA dropout kernels against the numpy mask (llava_mi355x/dropout.py) and float64.

  ops.dropout             (elementwise.hip)  bits: where(mask, T(x * fp32(1 / (1 - p))), +0)
  ops.dropout_add         (elementwise.hip)  bits: T(into + where(mask, t * scale, 0)) with the sum in fp32
  ops.lora_down_dropout   (lora.hip)         u_g = dropout_g(x) A_g^T against float64 of ops.dropout's output times A_g^T
  ops.lora_wgrad_dropout  (lora.hip)         dA = small^T dropout(big) against float64 of ops.dropout's output
The bound of the two products is the one tests/test_lora_wgrad_gpu.py derives, elementwise: |got - ref| <= u |ref| + 2 K 2^-24 sum_k |a b|, u = 2^-8 (bf16) /
2^-11 (f16), K = the contraction length (one rounding to the output dtype; the worst case of an fp32 sum in any order, doubled for the MFMA's internal rounding).
Operands and outputs are column windows of wider NaN-filled buffers: a read or a write outside a window shows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

P, SEED, STEP = 0.1, 0x0123_4567_89AB_CDEF, 5
COL0 = 8                                                  # the windows start 8 columns in: 16-byte aligned for every dtype
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _window(rows, cols, width, dtype, seed, device="cuda"):
    """A [rows, cols] window of N(0, 1) values inside a NaN-filled [rows + 4, width] buffer: (buffer, window)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.full((rows + 4, width), float("nan"), dtype=dtype)
    buf[:rows, COL0:COL0 + cols] = torch.randn((rows, cols), generator=g).to(dtype)
    buf = buf.to(device)
    return buf, buf[:rows, COL0:COL0 + cols]


def _mask(rows, cols, stream, step=STEP):
    from llava_mi355x import dropout as D
    return torch.from_numpy(D.keep_mask(P, SEED, step, stream, rows, cols))


def _restated(x, stream):
    """ops.dropout in torch on the CPU: the numpy mask and ONE rounding of the fp32 product."""
    from llava_mi355x import dropout as D
    xc = x.detach().cpu()
    scaled = (xc.float() * float(D.scale(P))).to(xc.dtype)
    return torch.where(_mask(*xc.shape, stream), scaled, torch.zeros_like(scaled))


def _outside_is_nan(buf, rows, cols):
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[:rows, COL0:COL0 + cols] = False
    return bool(torch.isnan(buf[outside]).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("rows,cols,width", [(64, 64, 64 + 2 * COL0), (192, 320, 384)])
def test_dropout_bits(cuda, rows, cols, width, dtype):
    from llava_mi355x import ops
    stream = 3 << 3 | 4
    _, x = _window(rows, cols, width, dtype, 1)
    obuf = torch.full((rows + 4, width), float("nan"), dtype=dtype, device=cuda)
    out = obuf[:rows, COL0:COL0 + cols]
    assert ops.dropout_ok(x, out)
    ops.dropout(x, P, SEED, STEP, stream, out=out)
    want = _restated(x, stream)
    assert torch.equal(_bits(out.cpu()), _bits(want))                       # bits: the sign of a dropped zero included
    assert _outside_is_nan(obuf, rows, cols)
    kept = float((out != 0).float().mean())
    assert 0.8 < kept < 0.97, kept
    again = ops.dropout(x, P, SEED, STEP, stream)                            # a pure function; a fresh contiguous output
    assert torch.equal(_bits(again), _bits(out))
    assert not torch.equal(ops.dropout(x, P, SEED, STEP + 1, stream), again) and not torch.equal(ops.dropout(x, P, SEED, STEP, stream + 1), again)
    inplace = x.clone()
    ops.dropout(inplace, P, SEED, STEP, stream, out=inplace)
    assert torch.equal(_bits(inplace), _bits(out))
    assert torch.equal(_bits(ops.dropout(x, 0.0, SEED, STEP, stream)), _bits(x))      # p = 0: the identity


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_dropout_add_bits(cuda, dtype):
    from llava_mi355x import dropout as D, ops
    rows, cols, stream = 192, 320, 1 << 16 | 2 << 3 | 6
    _, t = _window(rows, cols, 384, dtype, 2)
    ibuf, into = _window(rows, cols, 384, dtype, 3)
    before = into.detach().cpu().clone()
    ops.dropout_add(into, t, P, SEED, STEP, stream)
    add = torch.where(_mask(rows, cols, stream), t.cpu().float() * float(D.scale(P)), torch.zeros((rows, cols)))
    want = (before.float() + add).to(dtype)
    assert torch.equal(_bits(into.cpu()), _bits(want))
    assert _outside_is_nan(ibuf, rows, cols)


@functools.lru_cache(maxsize=None)
def _down_inputs(rows, K, dtype):
    """x window, one [256, K] factor (every Rp reads its first rows) and, per stream 0 .. 2, float64 of ops.dropout's output; computed once per shape."""
    from llava_mi355x import ops
    _, x = _window(rows, K, K + 64, dtype, 10 + rows + K)
    g = torch.Generator(device="cpu").manual_seed(rows * 3 + K)
    A = (torch.randn((256, K), generator=g) / K ** 0.5).to(dtype).cuda()
    xd = [ops.dropout(x, P, SEED, STEP, 40 + s).double() for s in range(3)]
    for s in range(3):
        assert torch.equal(xd[s].cpu(), _restated(x, 40 + s).double())       # the yardstick itself is the restated mask
    return x, A, xd


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("Rp", [64, 192])
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("rows", [64, 192])
def test_lora_down_dropout_matches_fp64_of_the_masked_input(cuda, rows, K, Rp, G, dtype):
    from llava_mi355x import ops
    x, A256, xd = _down_inputs(rows, K, dtype)
    A = A256[:Rp]
    A_stack = A.repeat(G, 1).contiguous()                  # the SAME factor G times: the windows of u differ through the masks alone
    ubuf = torch.full((rows + 4, G * Rp + 2 * COL0), float("nan"), dtype=dtype, device=cuda)
    u = ubuf[:rows, COL0:COL0 + G * Rp]
    assert x.stride(0) != K and ops.lora_down_dropout_ok(x, A_stack, G, out=u)
    ops.lora_down_dropout(x, A_stack, G, P, SEED, STEP, 40, out=u)
    assert _outside_is_nan(ubuf, rows, G * Rp)
    a64 = A.double()
    plain = x.double() @ a64.t()
    wins = []
    for g in range(G):
        got = u[:, g * Rp:(g + 1) * Rp].double()
        ref = xd[g] @ a64.t()
        tol = U[dtype] * ref.abs() + 2 * K * 2.0 ** -24 * (xd[g].abs() @ a64.abs().t())
        assert torch.isfinite(got).all(), g
        assert ((got - ref).abs() <= tol).all(), (g, ((got - ref).abs() - tol).max().item())
        ptol = U[dtype] * plain.abs() + 2 * K * 2.0 ** -24 * (x.double().abs() @ a64.abs().t())
        assert not ((got - plain).abs() <= ptol).all(), g                     # it is not the unmasked product
        wins.append(got)
    for i in range(G):
        for j in range(i + 1, G):
            assert not torch.equal(wins[i], wins[j]), (i, j)                  # every adapter under its own mask
    again = torch.empty((rows, G * Rp), dtype=dtype, device=cuda)
    ops.lora_down_dropout(x, A_stack, G, P, SEED, STEP, 40, out=again)
    assert torch.equal(again, u)


@functools.lru_cache(maxsize=None)
def _wgrad_inputs(rows, F, dtype):
    from llava_mi355x import ops
    _, big = _window(rows, F, F + 64, dtype, 20 + rows + F)
    _, small = _window(rows, 256, 256 + 32, dtype, 21 + rows + F)
    bd = ops.dropout(big, P, SEED, STEP, 77).double()
    return big, small, bd


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R", [64, 256])
@pytest.mark.parametrize("F", [64, 192])
@pytest.mark.parametrize("rows,n_slices", [(64, 0), (320, 2)])
def test_lora_wgrad_dropout_matches_fp64_of_the_masked_input(cuda, rows, n_slices, F, R, dtype):
    """320 rows over 2 slices = 3 + 2 K-steps: a slice-local row index in the mask would repeat rows 0 .. 127 in the second slice."""
    from llava_mi355x import ops
    big, small256, bd = _wgrad_inputs(rows, F, dtype)
    small = small256[:, :R]
    s64 = small.double()
    for transposed in (True, False):
        shape = (R, F) if transposed else (F, R)
        obuf = torch.full((shape[0] + 4, shape[1] + 2 * COL0), float("nan"), dtype=dtype, device=cuda)
        out = obuf[:shape[0], COL0:COL0 + shape[1]]
        assert ops.lora_wgrad_ok(big, small, out, transposed=transposed)
        ops.lora_wgrad_dropout(big, small, P, SEED, STEP, 77, out=out, transposed=transposed, n_slices=n_slices)
        ref, mag = bd.t() @ s64, bd.abs().t() @ s64.abs()                       # [F, R]
        plain = big.double().t() @ s64
        if transposed:
            ref, mag, plain = ref.t(), mag.t(), plain.t()
        tol = U[dtype] * ref.abs() + 2 * rows * 2.0 ** -24 * mag
        got = out.double()
        assert torch.isfinite(got).all() and _outside_is_nan(obuf, *shape)
        assert ((got - ref).abs() <= tol).all(), (transposed, ((got - ref).abs() - tol).max().item())
        assert not ((got - plain).abs() <= tol).all()
        out2 = torch.empty(shape, dtype=dtype, device=cuda)
        ops.lora_wgrad_dropout(big, small, P, SEED, STEP, 77, out=out2, transposed=transposed, n_slices=n_slices)
        assert torch.equal(out2, out)                                           # same inputs, same bits
        # the entry without the mask is untouched: it still gives the plain product
        ops.lora_wgrad(big, small, out2, transposed=transposed, n_slices=n_slices)
        pmag = big.double().abs().t() @ s64.abs()
        assert ((out2.double() - plain).abs() <= U[dtype] * plain.abs() + 2 * rows * 2.0 ** -24 * (pmag.t() if transposed else pmag)).all()


def test_fused_kernels_refuse_what_they_do_not_take(cuda):
    from llava_mi355x import _C, ops
    bf = torch.bfloat16
    x = torch.zeros((64, 128), dtype=bf, device=cuda)
    A = torch.zeros((64, 128), dtype=bf, device=cuda)
    assert ops.lora_down_dropout_ok(x, A, 1)
    assert not ops.lora_down_dropout_ok(x.float(), A.float(), 1)                                    # fp32: the materialising path
    assert not ops.lora_down_dropout_ok(x[:48], A, 1) and not ops.lora_down_dropout_ok(x[:, :96], A[:, :96], 1)
    assert not ops.lora_down_dropout_ok(x, A[:32], 1) and not ops.lora_down_dropout_ok(x, A.repeat(4, 1), 4)
    u = torch.full((64, 64), float("nan"), dtype=bf, device=cuda)
    sup = _C.lib.lmx_op_lora_down_dropout_supported
    for dt, rows, K, Rp, G in ((_C.DTYPE_F32, 64, 128, 64, 1), (_C.DTYPE_BF16, 48, 128, 64, 1), (_C.DTYPE_BF16, 64, 96, 64, 1), (_C.DTYPE_BF16, 64, 128, 32, 1),
                               (_C.DTYPE_BF16, 64, 128, 64, 4)):
        assert sup(dt, 128, 128, 64 * G, rows, K, Rp, G) == 0
        rc = _C.lib.lmx_op_lora_down_dropout(dt, _C.ptr(x), 128, _C.ptr(A), 128, _C.ptr(u), 64, rows, K, Rp, G, P, SEED, 0, 0, _C.stream_handle())
        assert rc != 0 and _C.last_error()
    for p in (-0.5, 1.0):
        with pytest.raises(ValueError):
            ops.dropout(x, p, SEED, 0, 0)
        rc = _C.lib.lmx_op_lora_down_dropout(_C.DTYPE_BF16, _C.ptr(x), 128, _C.ptr(A), 128, _C.ptr(u), 64, 64, 128, 64, 1, p, SEED, 0, 0, _C.stream_handle())
        assert rc != 0
        assert _C.lib.lmx_op_dropout(_C.DTYPE_BF16, _C.ptr(x), 128, _C.ptr(x), 128, 64, 128, p, SEED, 0, 0, _C.stream_handle()) != 0
    assert torch.isnan(u).all()                                                                     # errors, not launches
    assert not ops.dropout_ok(x[:, :36]) and ops.dropout_ok(x[:, 8:72])
