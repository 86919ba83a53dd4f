"""The accumulating forms of the gradient kernels (gradient accumulation: micro-batch i > 0 of an optimiser step adds to what the gradient buffer holds):

  lmx_op_gemm_wgrad_acc          (csrc/gemm8t.hip)  out = T(fp32(out) + dy^T x): the prior joins the fp32 accumulator in the epilogue, one rounding
  lmx_op_lora_wgrad_acc          (csrc/lora.hip)    out = T(alpha * big^T small + fp32(out)), in the reducer, both orientations
  lmx_op_lora_wgrad_dropout_acc  (csrc/lora.hip)    the same with the dropout mask on `big`
  lmx_op_cast_f32_add            (csrc/train.hip)   dst = T(fp32(dst) + src)

Yardsticks: the forward GEMM's residual epilogue (lmx_op_gemm with residual: `v += r; store4`, the same one-rounding sum on the same MFMA order) bit for bit, the
float64 bounds of tests/test_wgrad_gpu.py and tests/test_lora_wgrad_gpu.py with the prior inside the single rounding, torch's own fp32 add + cast bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _ops():
    from llava_mi355x import ops
    return ops


def _rand(shape, dtype, dev, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- gemm_wgrad ---------------------------------------------------------------------------------------------------------------------------------------------
WGRAD_SHAPES = [
    # rows, out features, in features
    (64, 256, 256),          # one K-step, one tile
    (192, 512, 256),         # three K-steps (the odd tail of the ring), two M-tiles
    (128, 256, 512),         # two N-tiles
    (512, 4096, 4352),       # 272 tiles: more workgroups than CUs
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,O,I", WGRAD_SHAPES)
def test_wgrad_acc_is_the_residual_epilogue_and_meets_fp64(cuda, rows, O, I, dtype):
    ops = _ops()
    dy = _rand((rows, O), dtype, cuda, 1, 0.5)
    x = _rand((rows, I), dtype, cuda, 2, 0.5)
    prior = _rand((O, I), dtype, cuda, 3)                                # N(0, 1) rounded to the dtype
    out = prior.clone()
    assert ops.wgrad_direct_ok(dy, x, out)
    ops.gemm_wgrad(dy, x, out, accumulate=True)
    old = ops.gemm(ops.transpose_padded(dy, 64), ops.transpose_padded(x, 64), residual=prior.clone(), variant=35)    # the existing one-rounding residual epilogue
    assert torch.equal(_bits(out), _bits(old))
    ref = dy.double().t() @ x.double() + prior.double()
    tol = U[dtype] * ref.abs().max().item() + 1e-6                       # the bound of test_wgrad_matches_fp64_and_the_two_transpose_path, prior inside the reference
    err = (out.double() - ref).abs().max().item()
    print(f"wgrad_acc {(rows, O, I)} {dtype}: max err {err:.3e} tol {tol:.3e}")
    assert torch.isfinite(out.float()).all()
    assert err <= tol
    # a zero prior gives the bits of the non-accumulating call
    plain = torch.full((O, I), float("nan"), dtype=dtype, device=cuda)
    ops.gemm_wgrad(dy, x, plain)
    zero = torch.zeros((O, I), dtype=dtype, device=cuda)
    ops.gemm_wgrad(dy, x, zero, accumulate=True)
    assert torch.equal(_bits(zero), _bits(plain))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_wgrad_acc_on_a_column_window_of_a_nan_buffer(cuda, dtype):
    """The operands of test_wgrad_on_column_windows_of_wider_buffers; out is a column window of a wider NaN-filled buffer with a finite prior inside the window: a
    prior load outside the window would bring a NaN in, a store outside would take one out."""
    ops = _ops()
    rows, O, I = 384, 512, 256
    big_dy = _rand((rows, 1280), dtype, cuda, 3); big_x = _rand((rows, 1024), dtype, cuda, 4)
    dy, x = big_dy[:, 768:768 + O], big_x[:, 512:512 + I]
    prior = _rand((O, I), dtype, cuda, 5)
    big_out = torch.full((O, 640), float("nan"), dtype=dtype, device=cuda)
    out = big_out[:, 128:128 + I]
    out.copy_(prior)
    assert ops.wgrad_direct_ok(dy, x, out)
    ops.gemm_wgrad(dy, x, out, accumulate=True)
    ref = dy.double().t() @ x.double() + prior.double()
    assert torch.isfinite(out.float()).all()
    assert (out.double() - ref).abs().max().item() <= U[dtype] * ref.abs().max().item()
    assert torch.equal(out, ops.gemm(ops.transpose_padded(dy.contiguous(), 64), ops.transpose_padded(x.contiguous(), 64), residual=prior.clone(), variant=35))
    assert torch.isnan(big_out[:, :128]).all() and torch.isnan(big_out[:, 128 + I:]).all()              # nothing outside the window was written


def test_wgrad_acc_structured_operands_give_exact_integers(cuda):
    """dy small integers, x one-hot in r, an integer prior, every sum below 256: out[o][i] = prior[o][i] + dy[perm[i]][o] exactly — a prior taken from another
    element (a transposed or shifted load) shows as a wrong integer."""
    ops = _ops()
    rows, O, I = 256, 256, 512
    r = torch.arange(rows, device=cuda)[:, None]; o = torch.arange(O, device=cuda)[None, :]
    dy = ((r * 3 + o * 5) % 127).to(torch.bfloat16)
    perm = torch.from_numpy(np.random.RandomState(0).permutation(I) % rows).to(cuda)
    x = torch.zeros((rows, I), dtype=torch.bfloat16, device=cuda)
    x[perm, torch.arange(I, device=cuda)] = 1.0                         # column i picks row perm[i]
    oo = torch.arange(O, device=cuda)[:, None]; ii = torch.arange(I, device=cuda)[None, :]
    prior = ((oo * 7 + ii * 11) % 128).to(torch.bfloat16)               # 126 + 127 < 256: every sum is exact in bf16
    out = prior.clone()
    ops.gemm_wgrad(dy, x, out, accumulate=True)
    want = (prior.float() + dy[perm, :].t().float()).to(torch.bfloat16)
    assert torch.equal(out, want)


def test_wgrad_acc_refuses_what_the_plain_entry_refuses(cuda):
    ops = _ops()
    from llava_mi355x._C import LmxError
    bf = torch.bfloat16
    for r, O, I, dt in ((64, 128, 256, bf), (64, 256, 320, bf), (32, 256, 256, bf), (64, 256, 256, torch.float32)):
        dy = torch.zeros((r, O), dtype=dt, device=cuda); x = torch.zeros((r, I), dtype=dt, device=cuda)
        out = torch.full((O, I), float("nan"), dtype=dt, device=cuda)
        assert not ops.wgrad_direct_ok(dy, x, out)
        with pytest.raises(LmxError):
            ops.gemm_wgrad(dy, x, out, accumulate=True)
        assert torch.isnan(out).all()                                   # an error, not a launch


# ---- lora_wgrad ---------------------------------------------------------------------------------------------------------------------------------------------
def _lora_acc_call(dt, big, small, rows, F, R, R_out, alpha, transposed, n_slices, out):
    from llava_mi355x import _C as C
    nbytes = int(C.lib.lmx_op_lora_wgrad_workspace(rows, F, R, n_slices))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    return C.lib.lmx_op_lora_wgrad_acc(dt, C.ptr(big), big.stride(0), C.ptr(small), small.stride(0), rows, F, R, R_out, alpha, int(transposed), n_slices, C.ptr(out),
                                       out.stride(0), C.ptr(ws), nbytes, C.stream_handle())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [64, 192])
@pytest.mark.parametrize("n_slices", [0, 1, 3])
@pytest.mark.parametrize("rows", [64, 320])
def test_lora_wgrad_acc_matches_fp64_inside_its_windows(cuda, rows, n_slices, F, dtype):
    """The windowed NaN buffers of tests/test_lora_wgrad_gpu.py; the output window holds a finite prior, everything around it (the columns at and past R_out
    included) is NaN.  |got - (prior + alpha ref)| <= u |prior + alpha ref| + alpha 2 rows 2^-24 mag: that file's bound with the prior inside the single rounding."""
    from llava_mi355x import _C as C
    from test_lora_wgrad_gpu import BIG_COL, RANKS, SMALL_COL, _inputs
    dt = C.torch_dtype_code(dtype)
    big_w, small_w, ref_full, mag_full = _inputs(rows, F, dtype)
    big = big_w[:rows, BIG_COL:BIG_COL + F]
    u, alpha = U[dtype], 0.25
    for R, R_out in RANKS:
        small = small_w[:rows, SMALL_COL:SMALL_COL + R]
        for transposed in (False, True):
            shape = (R_out, F) if transposed else (F, R_out)
            prior = _rand(shape, dtype, cuda, 100 + R + R_out + int(transposed))
            wide = torch.full((shape[0] + 2, shape[1] + 5), float("nan"), dtype=dtype, device=cuda)
            out = wide[1:1 + shape[0], 3:3 + shape[1]]
            out.copy_(prior)
            rc = _lora_acc_call(dt, big, small, rows, F, R, R_out, alpha, transposed, n_slices, out)
            assert rc == 0, C.last_error()
            ref = alpha * ref_full[:, :R_out]
            mag = mag_full[:, :R_out]
            if transposed:
                ref, mag = ref.t(), mag.t()
            ref = ref + prior.double()
            tol = u * ref.abs() + alpha * 2 * rows * 2.0 ** -24 * mag
            got = out.double()
            tag = (R, R_out, transposed)
            assert torch.isfinite(got).all(), tag
            assert ((got - ref).abs() <= tol).all(), (tag, ((got - ref).abs() - tol).max().item())
            outside = torch.ones_like(wide, dtype=torch.bool)
            outside[1:1 + shape[0], 3:3 + shape[1]] = False
            assert torch.isnan(wide[outside]).all(), tag         # nothing outside the output window was read into it or written
            wide2 = torch.full_like(wide, float("nan"))
            out2 = wide2[1:1 + shape[0], 3:3 + shape[1]]
            out2.copy_(prior)
            rc = _lora_acc_call(dt, big, small, rows, F, R, R_out, alpha, transposed, n_slices, out2)
            assert rc == 0 and torch.equal(_bits(out), _bits(out2)), tag       # the same call from the same prior: the same bits


@pytest.mark.parametrize("transposed", [False, True])
def test_lora_wgrad_acc_structured_operands_give_exact_integers(cuda, transposed):
    """big small integers, small one-hot in the rows, an integer prior, alpha = 1, every sum below 256: out[f][j] = prior + big[perm[j]][f] exactly."""
    ops = _ops()
    rows, F, R = 128, 192, 64
    r = torch.arange(rows, device=cuda)[:, None]; f = torch.arange(F, device=cuda)[None, :]
    big = ((r * 3 + f * 5) % 127).to(torch.bfloat16)
    perm = torch.from_numpy(np.random.RandomState(1).permutation(rows)[:R].copy()).to(cuda)
    small = torch.zeros((rows, R), dtype=torch.bfloat16, device=cuda)
    small[perm, torch.arange(R, device=cuda)] = 1.0
    ff = torch.arange(F, device=cuda)[:, None]; jj = torch.arange(R, device=cuda)[None, :]
    prior = ((ff * 7 + jj * 11) % 128).to(torch.bfloat16)               # [F, R]
    want = (prior.float() + big[perm, :].t().float()).to(torch.bfloat16)
    if transposed:
        prior, want = prior.t().contiguous(), want.t().contiguous()
    out = prior.clone()
    ops.lora_wgrad(big, small, out, transposed=transposed, accumulate=True)
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_lora_wgrad_dropout_acc_matches_fp64_of_the_masked_input(cuda, dtype):
    """The smallest shape of tests/test_lora_dropout_kernels_gpu.py (64 rows, F = 64, R = 64) and its masked float64 reference, plus the prior."""
    ops = _ops()
    from test_lora_dropout_kernels_gpu import COL0, P, SEED, STEP, _outside_is_nan, _wgrad_inputs
    rows, F, R = 64, 64, 64
    big, small256, bd = _wgrad_inputs(rows, F, dtype)
    small = small256[:, :R]
    s64 = small.double()
    for transposed in (True, False):
        shape = (R, F) if transposed else (F, R)
        prior = _rand(shape, dtype, cuda, 7 + int(transposed))
        obuf = torch.full((shape[0] + 4, shape[1] + 2 * COL0), float("nan"), dtype=dtype, device=cuda)
        out = obuf[:shape[0], COL0:COL0 + shape[1]]
        out.copy_(prior)
        ops.lora_wgrad_dropout(big, small, P, SEED, STEP, 77, out=out, transposed=transposed, accumulate=True)
        ref, mag = bd.t() @ s64, bd.abs().t() @ s64.abs()
        plain = big.double().t() @ s64
        if transposed:
            ref, mag, plain = ref.t(), mag.t(), plain.t()
        ref, plain = ref + prior.double(), plain + prior.double()
        tol = U[dtype] * ref.abs() + 2 * rows * 2.0 ** -24 * mag
        got = out.double()
        assert torch.isfinite(got).all() and _outside_is_nan(obuf, *shape)
        assert ((got - ref).abs() <= tol).all(), (transposed, ((got - ref).abs() - tol).max().item())
        assert not ((got - plain).abs() <= tol).all()                           # the mask took part


# ---- cast_f32_add -------------------------------------------------------------------------------------------------------------------------------------------
def _tie_pairs(dt):
    """(prior, src) with prior + src exactly half way between two adjacent finite values of the 16-bit dt (exact in fp32), both signs, subnormals included."""
    k = torch.arange(0, (1 << 15) - 1, 37, dtype=torch.int32)
    lo = k.to(torch.int16).view(dt)
    hi = (k + 1).to(torch.int16).view(dt)
    ok = torch.isfinite(lo.float()) & torch.isfinite(hi.float())
    lo, hi = lo[ok], hi[ok]
    half = (hi.float() - lo.float()) / 2
    return torch.cat([lo, -lo]), torch.cat([half, -half])


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_cast_f32_add_is_torchs_fp32_add_and_one_rounding(cuda, dt):
    """dst = T(fp32(dst) + src) against (dst.float() + src).to(dt) from torch, bit for bit: every pair of the special values (+-0, +-inf, NaN, fp32 and 16-bit
    subnormals, the f16 overflow edge), priors plus exactly half an ulp (round-half-to-even ties), random values; lengths 1, 255 and 4099."""
    ops = _ops()
    sp = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -149, -2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
                       2.0 ** -133, 2.0 ** -14, 65504.0, 65520.0, 16.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -11, -1.0, 1e38, 3e38], dtype=torch.float32)
    a, b = torch.meshgrid(sp, sp, indexing="ij")
    prior_parts, src_parts = [a.reshape(-1).to(dt)], [b.reshape(-1)]
    if dt != torch.float32:
        p, s = _tie_pairs(dt)
        prior_parts.append(p); src_parts.append(s)
    gen = torch.Generator().manual_seed(17)
    prior_parts.append(torch.randn(5000, generator=gen).to(dt)); src_parts.append(torch.randn(5000, generator=gen) * 2.0 ** -6)
    prior, src = torch.cat(prior_parts), torch.cat(src_parts)
    assert prior.numel() >= 4099
    for n in (1, 255, 4099, prior.numel()):
        pick = slice(0, n) if n == prior.numel() else slice(prior.numel() - 4099, prior.numel() - 4099 + n)     # the short ones from the ties / random part ...
        if n == 1:
            pick = slice(1, 2)                                                                                   # ... and one special pair: +0 + -0
        pr, sr = prior[pick], src[pick]
        want = (pr.float() + sr).to(dt)
        buf = torch.full((n + 8,), float("nan"), dtype=dt, device=cuda)
        buf[:n] = pr.to(cuda)
        ops.cast_f32(sr.to(cuda), buf[:n], accumulate=True)
        got = buf[:n].cpu()
        assert torch.isnan(buf[n:]).all()                                   # nothing past n was written
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), n
        diff = _bits(got)[~nan] != _bits(want)[~nan]
        assert not diff.any(), f"n = {n}: {int(diff.sum())} sums differ from torch, e.g. prior {pr[~nan][diff][:4].tolist()} src {sr[~nan][diff][:4].tolist()}"
