"""lmx_op_lora_wgrad (csrc/lora.hip): the gradient of one LoRA factor, out = alpha * big^T small with both operands in their forward layout (peft's lora_A / lora_B
are nn.Linear modules, so under the reference's LoRA fine-tune, llava/train/train.py:873-889, each is grad_output^T @ input of a linear r wide).

Through the C ABI, N(0, 1) inputs rounded to the dtype, against the float64 product of those rounded inputs.  The bound is derived, elementwise:
    |got - ref| <= u |ref| + 2 rows 2^-24 sum_row |big small|,      u = 2^-8 (bf16) / 2^-11 (f16)
(one rounding to the output dtype; the worst case of an fp32 sum in any order, doubled for the MFMA's internal rounding).
Shapes: the smallest that reach each seam — one K-step, an uneven split (320 rows = 5 K-steps over 2 or 3 slices), an automatic split above one (4096 rows,
F = 64), one and several column tiles, every rank width, ranks below the padded width, both orientations, both dtypes.  Operands and output are windows of wider
NaN-filled buffers, and the rows after `rows` are NaN: a read or a write outside the window shows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RANKS = [(64, 8), (64, 64), (128, 128), (256, 192)]          # (R = padded width read, R_out = columns stored)
BIG_COL, SMALL_COL, SMALL_W = 8, 16, 256 + 24


def _C():
    from llava_mi355x import _C
    return _C


@functools.lru_cache(maxsize=None)
def _inputs(rows, F, dtype):
    """Wide NaN-filled buffers with the operands as column windows, and the float64 references for the full 256-wide small operand (computed once per shape)."""
    g = torch.Generator(device="cpu").manual_seed(rows * 7 + F)
    big_w = torch.full((rows + 8, F + 16), float("nan"), dtype=dtype)
    small_w = torch.full((rows + 8, SMALL_W), float("nan"), dtype=dtype)
    big_w[:rows, BIG_COL:BIG_COL + F] = torch.randn((rows, F), generator=g).to(dtype)
    small_w[:rows, SMALL_COL:SMALL_COL + 256] = torch.randn((rows, 256), generator=g).to(dtype)
    big_w, small_w = big_w.cuda(), small_w.cuda()
    b64, s64 = big_w[:rows, BIG_COL:BIG_COL + F].double(), small_w[:rows, SMALL_COL:SMALL_COL + 256].double()
    ref = b64.t() @ s64                                         # [F, 256]: column j depends on small column j alone
    mag = b64.abs().t() @ s64.abs()
    return big_w, small_w, ref, mag


def _call(dt, big_w, small_w, rows, F, R, R_out, alpha, transposed, n_slices, out, ld_out=None):
    C = _C()
    big = big_w[:rows, BIG_COL:BIG_COL + F]
    small = small_w[:rows, SMALL_COL:SMALL_COL + R]
    nbytes = int(C.lib.lmx_op_lora_wgrad_workspace(rows, F, R, n_slices))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = C.lib.lmx_op_lora_wgrad(dt, C.ptr(big), big.stride(0), C.ptr(small), small.stride(0), rows, F, R, R_out, alpha, int(transposed), n_slices, C.ptr(out),
                                 out.stride(0) if ld_out is None else ld_out, C.ptr(ws), nbytes, C.stream_handle())
    return rc, nbytes


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("F", [64, 192, 384])
@pytest.mark.parametrize("n_slices", [0, 1, 2, 3])
@pytest.mark.parametrize("rows", [64, 320, 4096])
def test_lora_wgrad_matches_fp64_inside_its_windows(cuda, rows, n_slices, F, dtype):
    C = _C()
    dt = C.torch_dtype_code(dtype)
    big_w, small_w, ref_full, mag_full = _inputs(rows, F, dtype)
    u = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    alpha = 0.25                                                 # a power of two: scaling the reference by it is exact
    for R, R_out in RANKS:
        for transposed in (False, True):
            shape = (R_out, F) if transposed else (F, R_out)
            wide = torch.full((shape[0] + 2, shape[1] + 5), float("nan"), dtype=dtype, device=cuda)
            out = wide[1:1 + shape[0], 3:3 + shape[1]]
            assert C.lib.lmx_op_lora_wgrad_supported(dt, big_w.stride(0), small_w.stride(0), rows, F, R, R_out, int(transposed), out.stride(0)) == 1
            rc, nbytes = _call(dt, big_w, small_w, rows, F, R, R_out, alpha, transposed, n_slices, out)
            assert rc == 0, C.last_error()
            if rows == 4096 and F == 64 and n_slices == 0:
                assert nbytes > F * R * 4                        # the automatic split takes more than one slice here
            ref = alpha * ref_full[:, :R_out]
            tol = u * ref.abs() + alpha * 2 * rows * 2.0 ** -24 * mag_full[:, :R_out]
            if transposed:
                ref, tol = ref.t(), tol.t()
            got = out.double()
            tag = (R, R_out, transposed)
            assert torch.isfinite(got).all(), tag                # no NaN from outside a window, no pad column, every element written
            assert ((got - ref).abs() <= tol).all(), (tag, ((got - ref).abs() - tol).max().item())
            outside = torch.ones_like(wide, dtype=torch.bool)
            outside[1:1 + shape[0], 3:3 + shape[1]] = False
            assert torch.isnan(wide[outside]).all(), tag         # nothing outside the output window was written
            wide2 = torch.full_like(wide, float("nan"))
            out2 = wide2[1:1 + shape[0], 3:3 + shape[1]]
            rc, _ = _call(dt, big_w, small_w, rows, F, R, R_out, alpha, transposed, n_slices, out2)
            assert rc == 0 and torch.equal(out, out2), tag       # same inputs, same bits


def test_lora_wgrad_refuses_what_it_does_not_take(cuda):
    C = _C()
    bf = C.DTYPE_BF16
    sup = lambda dt, rows, F, R, R_out=None, ld_big=None: C.lib.lmx_op_lora_wgrad_supported(dt, ld_big or F, R, rows, F, R, R if R_out is None else R_out, 0, R)
    assert sup(bf, 64, 64, 64) == 1 and sup(C.DTYPE_F16, 128, 192, 256, 192) == 1
    assert sup(bf, 64, 72, 64) == 0 and sup(bf, 96, 64, 64) == 0 and sup(bf, 64, 64, 32) == 0 and sup(C.DTYPE_F32, 64, 64, 64) == 0
    assert sup(bf, 64, 64, 64, 65) == 0 and sup(bf, 64, 64, 64, 0) == 0 and sup(bf, 64, 64, 64, None, 68) == 0
    for dt, rows, F, R in ((bf, 64, 72, 64), (bf, 96, 64, 64), (bf, 64, 64, 32), (C.DTYPE_F32, 64, 64, 64)):
        big = torch.zeros((128, 128), dtype=torch.bfloat16, device=cuda); small = torch.zeros((128, 64), dtype=torch.bfloat16, device=cuda)
        out = torch.full((128, 64), float("nan"), dtype=torch.bfloat16, device=cuda); ws = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
        rc = C.lib.lmx_op_lora_wgrad(dt, C.ptr(big), 128, C.ptr(small), 64, rows, F, R, R, 1.0, 0, 0, C.ptr(out), 64, C.ptr(ws), ws.numel(), C.stream_handle())
        assert rc != 0 and C.last_error()
        assert torch.isnan(out).all()                           # an error, not a launch


def test_ops_wrapper_takes_the_two_gradients_of_a_linear(cuda):
    """ops.lora_wgrad as the training step calls it: dB = s dy^T u ([out, r]) and dA = du^T x ([r, in], transposed), r = 8 stored from a 64-wide padded operand."""
    from llava_mi355x import ops
    g = torch.Generator(device="cpu").manual_seed(5)
    rows, I, O, r = 128, 192, 320, 8
    x = torch.randn((rows, I), generator=g).to(torch.bfloat16).cuda(); dy = torch.randn((rows, O), generator=g).to(torch.bfloat16).cuda()
    u = torch.zeros((rows, 64), dtype=torch.bfloat16, device=cuda); u[:, :r] = torch.randn((rows, r), generator=g).to(torch.bfloat16).cuda()
    dB = torch.zeros((O, 64), dtype=torch.bfloat16, device=cuda)
    assert ops.lora_wgrad_ok(dy, u, dB) and ops.lora_wgrad_ok(x, u, torch.empty((64, I), dtype=torch.bfloat16, device=cuda), transposed=True)
    ops.lora_wgrad(dy, u, dB, alpha=2.0)
    ref = 2.0 * dy.double().t() @ u.double()
    assert ((dB.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2 * rows * 2.0 ** -23 * (dy.double().abs().t() @ u.double().abs())).all()
    assert dB[:, r:].abs().max().item() == 0                    # products with zero columns are exactly zero
    dA = ops.lora_wgrad(x, u, r_out=r, transposed=True)
    ref = u[:, :r].double().t() @ x.double()
    assert tuple(dA.shape) == (r, I)
    assert ((dA.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2 * rows * 2.0 ** -24 * (u[:, :r].double().abs().t() @ x.double().abs())).all()
    assert not ops.lora_wgrad_ok(x.float(), u.float(), torch.empty((64, I), device=cuda), transposed=True)
