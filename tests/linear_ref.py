"""float64 statements of the project's linears (the decode GEMV family and the GEMMs) with per-element error bounds that are DERIVED from the kernels' arithmetic,
never fitted to their output.  Shared by test_linears_fp64_gpu.py, test_ops_gpu.py and test_batching_gpu.py; ulp_of / assert_one_ulp live in test_gemm8p_gpu.py.

Everything stays on the device the inputs are on (the float64 copy of a 22016 x 4096 weight is 0.7 GB)."""
import math

import torch

from test_gemm8p_gpu import DT, assert_one_ulp, ulp_of  # noqa: F401  (re-exported)

U = 2.0 ** -24                       # unit roundoff of fp32: one rounding of an fp32 add / mul / fma moves the result by at most U |result|
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SILU_MUL = 0, 1, 2, 3
FLIP_REL = 2.0 ** -21                # how far the kernel's fp32 `inv` (fp32 mean of squares, rsqrtf) is taken to stand from the float64 one
FLIP_MAX_FRACTION = 0.01             # the flippable set is a cap that could hide a failure: it may hold at most 1 % of K


def rnd(v64, dt):
    """A float64 tensor rounded to the storage dtype, as float64."""
    return v64.to(DT[dt]).double()


def act64(y, act):
    """(act(y), |act'(y)|, act_n) in float64.  act_n bounds what the kernel's fast-math evaluation of act adds in fp32:

    * quick-GELU y / (1 + __expf(-1.702 y)) and SiLU y / (1 + __expf(-y)): __expf(v) is v_exp_f32(v * log2 e); the HIP math API reference lists the intrinsic at
      1 ulp (= 2 U relative) for an exact argument, the fp32 products in front of it (1.702 y, then * log2 e) move the argument by 2 |v| U, which the exponential turns
      into a relative error of the same size: rel(e) = (2 + 2 |v|) U.  d act / d e = -y / (1 + e)^2, so that is |y| e / (1 + e)^2 * rel(e); the add 1 + e (U) and
      the fp32 division (correctly rounded without fast-math; taken as 3 U in case it is lowered to v_rcp_f32 and a product) add 4 U |act|.
    * GELU-erf 0.5 y erfcf(-y / sqrt 2): erfcf is an OCML function held to the OpenCL full-profile limit of 16 ulp = 32 U relative (OpenCL C 1.2 section 7.4; the HIP
      math API reference lists a smaller figure, the larger one is used); the argument t = -y / sqrt 2 carries 2 U (the constant and the product), d ln erfc / d ln t
      is at most 2 t^2 + 1, and the two products add 2 U: (32 + 2 (2 t^2 + 1) + 2) U |act|."""
    if act == ACT_NONE:
        return y, torch.ones_like(y), torch.zeros_like(y)
    if act in (ACT_QUICK_GELU, ACT_SILU_MUL):
        s = 1.702 if act == ACT_QUICK_GELU else 1.0
        sg = torch.sigmoid(s * y)
        f = y * sg
        d = sg + s * y * sg * (1 - sg)
        n = y.abs() * sg * (1 - sg) * (2 + 2 * (s * y).abs()) * U + 4 * U * f.abs()          # e / (1 + e)^2 = sg (1 - sg)
        return f, d.abs(), n
    if act == ACT_GELU_ERF:
        t = y / math.sqrt(2.0)
        Phi = 0.5 * torch.erfc(-t)
        f = y * Phi
        d = Phi + y * torch.exp(-0.5 * y * y) / math.sqrt(2 * math.pi)
        n = f.abs() * (32 + 2 * (2 * t * t + 1) + 2) * U
        return f, d.abs(), n
    raise ValueError(act)


def norm_chain(x, dt, eps):
    """(x inv64 in float64, the mask of elements whose round_T the kernel's fp32 inv can move) for the RMSNorm prologue of x [M, K]."""
    xd = x.double()
    e32 = float(torch.tensor(eps, dtype=torch.float32))                          # the entry point takes eps as a float
    p = xd / torch.sqrt(xd.pow(2).mean(-1, keepdim=True) + e32)
    if dt == "f32":
        return p, torch.zeros_like(p, dtype=torch.bool)
    return p, rnd(p * (1 - FLIP_REL), dt) != rnd(p * (1 + FLIP_REL), dt)


def flip_fraction(x, dt, eps=1e-5):
    """The largest share, over the rows of x, of elements in the flippable set."""
    return float(norm_chain(x, dt, eps)[1].double().mean(-1).max())


def _through_act(y, dy, act):
    """act(y) and the bound on |act_kernel(y + e) - act(y)| for |e| <= dy: first order |act'(y)| dy, second order dy^2 (|act''| <= 1.2 for all three, halved by
    Taylor's 1/2, rounded up to 1), plus the evaluation error act_n."""
    f, d, n = act64(y, act)
    if act == ACT_NONE:
        return f, dy
    return f, d * dy + dy * dy + n


def linear_ref(x, w, dt, bias=None, residual=None, norm_w=None, eps=1e-5, act=ACT_NONE, chain=None, tree=6):
    """float64 reference and per-element bound for   out = round_T( act(xs . w + bias) + residual ),   xs = x or round_T(round_T(x inv) g).

    x [M, K], w [N, K] (for SiLU*mul: the gate rows and the up rows as a PAIR (wg, wu) of [I, K] tensors).  Returns (ref64, E, flip_fraction) with
        |got - round_T(ref64)| <= ulp_T(ref64) + E        for an implementation with the kernels' arithmetic:

    * fp32 fmaf chain of `chain` terms per lane (default: the GEMV kernels' 8 elements x ceil(K / 8 / 64) rounds), then `tree` levels of pairwise fp32 adds
      (wave_sum: 6).  Worst case of recursive summation (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4 with fused multiply-adds: one
      rounding per term): |sum_fp32 - sum| <= (chain + tree) U sum_k |xs_k w_nk|.
    * the epilogue in fp32: `+ bias` (one rounding, U |y + b|), the activation (see act64), `+ residual` (one rounding, U |out|); ONE rounding to T at the end.
    * T = float with a norm prologue: xs itself is an fp32 chain (x * inv rounded, * g rounded: 2 U) on an `inv` that stands FLIP_REL = 8 U from the float64 one:
      10 more units on the chain.
    * T = bf16 / f16 with a norm prologue: the two products are exact in fp32 (8 + 8 and 11 + 11 significand bits), so xs matches the float64 chain exactly EXCEPT
      where x_k inv sits so close to a rounding boundary of T that the kernel's inv puts it on the other side.  Those k are marked — round_T(x_k inv64 (1 - 2^-21))
      != round_T(x_k inv64 (1 + 2^-21)) — and each adds 2 ulp_T(xs_k) |w_nk| (one ulp of the first rounding carried through g, one for the second rounding landing
      elsewhere).  flip_fraction = the largest marked share of K over the rows; the caller asserts it <= FLIP_MAX_FRACTION."""
    M, K = x.shape
    if chain is None:
        chain = 8 * ((K // 8 + 63) // 64)
    units = chain + tree
    xd = x.double()
    flip_w = None
    flip_fraction = 0.0          # shadows the module function inside this body only
    if norm_w is not None:
        p, flip = norm_chain(x, dt, eps)
        xs = rnd(rnd(p, dt) * norm_w.double(), dt)
        if dt == "f32":
            units += 10
        else:
            flip_fraction = float(flip.double().mean(-1).max())
            flip_w = flip.double() * 2 * ulp_of(xs, dt)
    else:
        xs = xd
    gamma = units * U

    def pre(wpart, bpart):
        wd = wpart.double()
        y = xs @ wd.t()
        wa = wd.abs_()                                                           # in place: wd is not needed again
        dy = gamma * (xs.abs() @ wa.t())
        if flip_w is not None:
            dy = dy + flip_w @ wa.t()
        del wd, wa
        if bpart is not None:
            y = y + bpart.double()
            dy = dy + U * y.abs()
        return y, dy

    if act == ACT_SILU_MUL:
        wg, wu = w
        bg, bu = bias if bias is not None else (None, None)
        g, dg = pre(wg, bg)
        u, du = pre(wu, bu)
        s, ds = _through_act(g, dg, ACT_SILU_MUL)
        ref = s * u
        E = ds * (u.abs() + du) + s.abs() * du + U * ref.abs()                   # silu(g) * u: both factors off, one rounding of the product
        return ref, E, flip_fraction
    y, dy = pre(w, bias)
    ref, E = _through_act(y, dy, act)
    if residual is not None:
        ref = ref + residual.double()
        E = E + U * ref.abs()
    return ref, E, flip_fraction


def check(got, ref, E, dt, what=""):
    """assert |got - round_T(ref)| <= ulp_T(ref) + E for every element; returns the worst err / bound (informational)."""
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    gd = got.double()
    assert torch.isfinite(gd).all(), f"{what}: non-finite outputs"
    err = (gd - rnd(ref, dt)).abs()
    bound = ulp_of(ref, dt) + E
    ratio = err / bound
    worst = float(ratio.max())
    n_bad = int((err > bound).sum())
    if n_bad:
        i = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {n_bad} of {err.numel()} outputs outside ulp_T(ref) + derived fp32 bound; worst {worst:.2f}x at flat index {i}: "
                             f"got {float(gd.flatten()[i])!r}, float64 {float(ref.flatten()[i])!r}, bound {float(bound.flatten()[i]):.3e}")
    return worst


def gemm16_check(got, ref, dt, activated, what=""):
    """The 16-bit MFMA GEMMs: one ulp of the once-rounded float64 result plus the project's accumulation-noise constants of test_gemm8p_gpu.py (2e-5 of max |ref|
    plain, 3e-5 with an activation: they only matter for results that cancel to ~0)."""
    assert torch.isfinite(got.float()).all(), f"{what}: non-finite outputs"
    return assert_one_ulp(got, ref, dt, (3e-5 if activated else 2e-5) * float(ref.abs().max()), what)


def gemm16_gelu_tail_check(got, y, dt, what=""):
    """bias + GELU-erf WITHOUT a residual in a 16-bit MFMA GEMM, held per element to a bound that is relative where |ref| is small (gemm16_check's constant of
    3e-5 max |ref| is a hundred times |gelu(-5)|, and a residual of order 1 hides the tail behind its own ulp).  y: the float64 pre-activations.

    * accumulation noise enters BEFORE the activation: dy = 2e-5 max |y| (the project's constant, applied where the noise arises) reaches the output as
      |gelu'(y)| dy + dy^2 — at y = -6 that is 1e-7, not 3e-4;
    * the MFMA epilogues evaluate 0.5 y (1 + erff(y / sqrt 2)) (common.h: act_gelu_erf; they keep the parent's bits).  In fp32: erff within the OpenCL limit of
      16 ulp of a value below 1 (16 U absolute), its argument off by 2 U |t| (under 1 U through erf' t), the sum 1 + erf rounded once (U, the sum is below 2):
      18 U absolute on the sum, times 0.5 |y|, and two products (2 U |gelu|):   9 U |y| + 2 U |gelu(y)|.
      This is the cancellation of that form stated as a bound — 3e-6 at y = -6, where gelu is 6e-9 — so what it leaves is asserted, not absorbed."""
    f, d, _ = act64(y, ACT_GELU_ERF)
    dy = 2e-5 * float(y.abs().max())
    E = d * dy + dy * dy + 9 * U * y.abs() + 2 * U * f.abs()
    return check(got, f, E, dt, what)
