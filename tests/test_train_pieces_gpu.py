"""The pieces of one optimisation step that the whole-step tests cannot see (csrc/train.hip, composed by llava_mi355x/train.py): AdamW with the
global-norm clip, the squared-norm reduction, the elementwise ops with HF's rounding points, the fp32 -> parameter-dtype cast, the bias-gradient
column sums, and the embedding gather (csrc/elementwise.hip) with its gradient.

Every test goes through llava_mi355x.ops (the C ABI) and compares with float64 computed from the values the kernel actually read (16-bit and fp32
values are exact in float64; scalar hyperparameters are taken as the fp32 values the C ABI passes).  Output buffers start as NaN, so an element the
kernel never writes fails.  Each docstring states its tolerance and where it comes from; u = 2^-24 is the unit roundoff of fp32, and a chain of d
fp32 roundings moves a result by at most gamma_d = d u / (1 - d u) relative to the sum of the magnitudes it adds."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MANT = {torch.float32: 24, torch.bfloat16: 8, torch.float16: 11}          # significand bits incl. the hidden one
IBITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def _ops():
    from llava_mi355x import ops
    return ops


def _err():
    from llava_mi355x._C import LmxError
    return LmxError


def _bits(t):
    return t.view(IBITS[t.dtype])


def _ulp(ref64, dt):
    """Spacing of dt at |ref| (float64 tensor), clamped at the smallest normal (below it: the subnormal spacing)."""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(torch.finfo(dt).tiny)))
    return torch.pow(2.0, e - (MANT[dt] - 1))


def _gam(d):
    return d * U / (1 - d * U)


def _f32(x):
    """x as the fp32 scalar the C ABI passes."""
    return float(np.float32(x))


# ---- AdamW ------------------------------------------------------------------------------------------------------------------------------------
ADAM_N = 256 * 37 + 5                       # 37 full workgroups and a partial one
ADAM_STEPS = [
    # lr, gnorm_sq (None: no device scalar), max_grad_norm          clip = min(1, max / (sqrt(gnorm_sq) + 1e-6))
    (0.1, 400.0, 1.0),                      # 0.05
    (0.03, 0.25, 1.0),                      # norm 0.5 below the maximum: 1
    (0.2, (2.0 / 0.3) ** 2, 2.0),           # 0.3
    (0.05, None, 1.0),                      # no norm scalar: unclipped
    (0.15, 400.0, 0.0),                     # max_grad_norm 0: no clipping although a scalar is passed
    (0.07, 6.25, 1.5),                      # 0.6
]
MUTATIONS = ("ignore_gnorm", "clip_m_only", "eps_in_sqrt", "eps_before_bc2", "wd_after_update", "wd_without_lr", "bc2_not_sqrt", "swap_betas")
ADAM_RUNS = {
    # first step, betas, eps, weight decay, the mistakes this run must expose
    "fresh_wd": (1, (0.9, 0.999), 1e-8, 0.1, MUTATIONS),
    "fresh_big_eps": (1, (0.8, 0.95), 1e-3, 0.0, tuple(m for m in MUTATIONS if not m.startswith("wd"))),
    "late_wd_big_eps": (1000, (0.9, 0.999), 1e-3, 0.1, MUTATIONS),
    "late_beta2_095": (1000, (0.8, 0.95), 1e-8, 0.1, tuple(m for m in MUTATIONS if m not in ("eps_before_bc2", "bc2_not_sqrt"))),
}


def _clip(gnorm_sq, max_norm):
    return 1.0 if gnorm_sq is None or max_norm <= 0 else min(1.0, max_norm / (math.sqrt(gnorm_sq) + 1e-6))


def _adamw64(p0, m0, v0, g, lr, b1, b2, eps, wd, t, clip, mut=None):
    """One AdamW step in float64 in torch.optim.AdamW's order, or the same step with the mistake `mut`.  Returns p, m, v and the intermediate
    values the error bound needs."""
    if mut == "swap_betas":
        b1, b2 = b2, b1
    gc = g * (1.0 if mut == "ignore_gnorm" else clip)
    gv = g if mut == "clip_m_only" else gc
    p1 = p0 if mut == "wd_after_update" else p0 * (1 - (wd if mut == "wd_without_lr" else lr * wd))
    A, B = b1 * m0, (1 - b1) * gc
    C, D = b2 * v0, (1 - b2) * gv * gv
    m, v = A + B, C + D
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    bc2s = bc2 if mut == "bc2_not_sqrt" else math.sqrt(bc2)
    if mut == "eps_in_sqrt":
        den = torch.sqrt(v / bc2 + eps)
    elif mut == "eps_before_bc2":
        den = (torch.sqrt(v) + eps) / bc2s
    else:
        den = torch.sqrt(v) / bc2s + eps
    step = (lr / bc1) * (m / den)
    p = p1 - step
    if mut == "wd_after_update":
        p = p * (1 - lr * wd)
    return p, m, v, dict(A=A, B=B, C=C, D=D, bc1=bc1, bc2=bc2, den=den, step=step)


def _adamw_bound(p0, p, v, parts, lr, b1, b2, wd, t, dg):
    """Per-element bounds (master, exp_avg, exp_avg_sq) on adamw_kernel's fp32 evaluation; derived in test_adamw_matches_torch_adamw_in_float64."""
    A, B, C, D = (parts[k].abs() for k in "ABCD")
    bc1, bc2, den, step = parts["bc1"], parts["bc2"], parts["den"], parts["step"]
    bm = 2 * U * A + (dg + 2 * U) * B
    bv = 2 * U * C + (2 * dg + 3 * U) * D
    e1 = 2 * U * b1 ** t / bc1 + U
    e2 = 2 * U * b2 ** t / bc2 + U
    s = torch.sqrt(v) / math.sqrt(bc2)
    ev = torch.where(v > 0, bv / v.clamp_min(1e-300), torch.zeros_like(v))
    rden = (s * (ev / 2 + e2 / 2 + 3 * U) + U * den) / den
    dstep = step.abs() * (e1 + rden + 3 * U) + (lr / bc1) * bm / den
    dp = (3 * U * p0.abs() if wd > 0 else 0) + dstep + U * p.abs()
    tiny = 2.0 ** -147                      # a few fp32 subnormal spacings
    return 2 * dp + tiny, 2 * bm + tiny, 2 * bv + tiny


def _torch_adamw(params, grads, ms, vs, lr, betas, eps, wd, t):
    """torch.optim.AdamW on float64 CPU tensors from the given state (step t - 1 done); returns the updated (params, exp_avgs, exp_avg_sqs)."""
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    for p, m, v in zip(ps, ms, vs):
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    opt.step()
    return [p.detach() for p in ps], [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]


def _adam_grads(n, dt, seed):
    """Gradients of magnitude 1e-10 .. 1e2 (log-uniform, both signs) with 3 % exact zeros, as stored in dt (f16 takes the smallest to its
    subnormals or to zero: the test uses the stored values)."""
    gen = torch.Generator().manual_seed(seed)
    g = torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 12 - 10)
    g = torch.where(torch.rand(n, generator=gen) < 0.5, -g, g)
    g[torch.rand(n, generator=gen) < 0.03] = 0.0
    return g.to(dt)


@pytest.mark.parametrize("run", list(ADAM_RUNS))
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_adamw_matches_torch_adamw_in_float64(cuda, dt, run):
    """lmx_op_adamw over six consecutive steps on one device state (master, exp_avg, exp_avg_sq): clip factors 0.05, 1, 0.3, no norm scalar,
    max_grad_norm 0 and 0.6, a different lr on every step, from step 1 or from preloaded moments at step 1000.  Each step is compared with
    torch.optim.AdamW in float64 started from the state the kernel stored, with p.grad = g * clip (what clip_grad_norm_ leaves), and `param` must be
    the RNE rounding of the kernel's own master, bit for bit.

    Bound (first order in u, per element).  The kernel reads exact inputs and rounds each operation once:
      g * clip: sqrt, + 1e-6, divide, multiply -> relative dg = 5u;
      m = b1 m0 + (1 - b1) g (1 - b1 exact by Sterbenz): |dm| <= 2u |b1 m0| + (dg + 2u) |(1 - b1) g|;
      v = b2 v0 + ((1 - b2) g) g:                        |dv| <= 2u |b2 v0| + (2 dg + 3u) (1 - b2) g^2;
      bc = 1 - powf(b, t) on the host (powf within 1 ulp <= 2u b^t, one rounding of the difference): relative e = 2u b^t / bc + u;
      s = sqrt(v) / sqrt(bc2): relative dv / 2v + e2 / 2 + 3u;  den = s + eps: |dden| <= s rel(s) + u den;
      step = (lr / bc1) (m / den): |dstep| <= |step| (e1 + rel(den) + 3u) + (lr / bc1) |dm| / den;
      p = p0 (1 - lr wd) - step: |dp| <= 3u |p0| (wd > 0) + |dstep| + u |p|.
    FMA contraction only removes roundings.  The asserted bound is twice this sum (the second-order terms are products of two relative errors,
    below 1e-9 of it) plus 2^-147 for subnormal results.

    Every mistake in MUTATIONS is evaluated from the same stored state and must leave the reference by at least 10x this bound somewhere in the six
    steps: the test asserts it, so the ratios are checked, not just claimed.  The arithmetic behind them (lr ~ 0.1, |p0| ~ 0.5, bound on p
    ~ 1e-7 |p0| + 1e-6 |step|, bounds on m and v ~ 10u of their terms):
      ignore gnorm_sq (clip 0.05 / 0.3 / 0.6 dropped): m moves by (1 - b1) |g| (1 - clip), ratio ~ (1 - clip) / (7u clip) > 1e5;
      clip m but not v: v moves by (1 - b2) g^2 (1 - clip^2), ratio ~ 1 / (13u) where (1 - b2) g^2 dominates b2 v0 (every element at step 1);
      eps inside the sqrt: den = sqrt(v / bc2 + eps) >= sqrt(1e-8) = 1e-4 instead of ~ |g| + eps, so the steps of the |g| < 1e-5 elements shrink
        10 - 1e4x: dp ~ lr = 0.1 against ~ 1e-7;
      eps before the sqrt(1 - b2^t) division: den grows by eps (1 / sqrt(bc2) - 1) = 30 eps at t = 1 (b2 = 0.999), 0.26 eps at t = 1000; the
        elements with sqrt(v / bc2) ~ eps change their step by O(1): dp ~ lr against ~ 1e-7 (invisible once b2^t underflows: bc2 = 1, run
        late_beta2_095);
      weight decay after the update: dp = lr wd |step| ~ 0.1 * 0.1 * 0.1 = 1e-3; without lr: dp = wd (1 - lr) |p0| ~ 0.05 (runs with wd = 0.1);
      bc2 not square-rooted: the step scales by sqrt(bc2) = 0.03 (t = 1) ... 0.8 (t = 1000): dp ~ lr (again invisible once bc2 = 1);
      beta1 <-> beta2: m = 0.999 m0 + 0.001 g instead of 0.9 m0 + 0.1 g: m changes by ~ 100 %, ratio ~ 1 / u."""
    ops = _ops()
    t0, betas, eps, wd, must_catch = ADAM_RUNS[run]
    b1, b2, eps32, wd32 = _f32(betas[0]), _f32(betas[1]), _f32(eps), _f32(wd)
    n = ADAM_N
    gen = torch.Generator().manual_seed(7 + t0)
    master = (torch.randn(n, generator=gen) * 0.5).to(cuda)
    if t0 == 1:
        m = torch.zeros(n, device=cuda)
        v = torch.zeros(n, device=cuda)
    else:                                   # moments of a long run: |m| <= sqrt(v), magnitudes over many decades
        m64 = torch.randn(n, generator=gen, dtype=torch.float64) * torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 10 - 9)
        m = m64.float().to(cuda)
        v = (m64 * m64 * torch.pow(10.0, torch.rand(n, generator=gen, dtype=torch.float64) * 4) + 1e-24).float().to(cuda)
    param = torch.empty(n, dtype=dt, device=cuda)
    worst = {k: 0.0 for k in MUTATIONS}
    for i, (lr, gsq, max_norm) in enumerate(ADAM_STEPS):
        t, lr32 = t0 + i, _f32(lr)
        g = _adam_grads(n, dt, 100 * i + t0).to(cuda)
        gn = None if gsq is None else torch.tensor([gsq], dtype=torch.float32, device=cuda)
        p0, m0, v0, g64 = (x.double().cpu() for x in (master, m, v, g))
        clip = _clip(None if gsq is None else _f32(gsq), _f32(max_norm))
        param.fill_(float("nan"))
        ops.adamw(param, g, master, m, v, lr, betas, eps, wd, t, gnorm_sq=gn, max_grad_norm=max_norm)
        torch.cuda.synchronize()
        (pw,), (mw,), (vw,) = _torch_adamw([p0], [g64 * clip], [m0], [v0], lr32, (b1, b2), eps32, wd32, t)
        p64, m64, v64, parts = _adamw64(p0, m0, v0, g64, lr32, b1, b2, eps32, wd32, t, clip)
        bounds = _adamw_bound(p0, p64, v64, parts, lr32, b1, b2, wd32, t, 5 * U)
        for name, a, w, bd in zip(("p", "m", "v"), (p64, m64, v64), (pw, mw, vw), bounds):
            assert ((a - w).abs() <= 1e-3 * bd).all(), f"step {t}: the float64 formula of this test disagrees with torch.optim.AdamW on {name}"
        for name, x, w, bd in zip(("master", "exp_avg", "exp_avg_sq"), (master, m, v), (pw, mw, vw), bounds):
            x = x.double().cpu()
            assert torch.isfinite(x).all(), f"step {t}: non-finite {name}"
            r = (x - w).abs() / bd
            assert r.max().item() <= 1.0, f"step {t}: {name} is {r.max().item():.3g}x the bound at element {int(r.argmax())}"
        assert torch.equal(_bits(param), _bits(master.to(dt))), f"step {t}: param is not the rounded master"
        for mut in MUTATIONS:
            got = _adamw64(p0, m0, v0, g64, lr32, b1, b2, eps32, wd32, t, clip, mut)[:3]
            worst[mut] = max([worst[mut]] + [((x - w).abs() / bd).max().item() for x, w, bd in zip(got, (pw, mw, vw), bounds)])
    missed = {k: worst[k] for k in must_catch if not worst[k] >= 10}
    assert not missed, f"mistakes that would stay within 10x of the bound: {missed}"


def _sumsq_depth(n):
    """Roundings on the longest path of a term through sumsq_kernel: 8 per 8-element chunk a thread walks (one fma each), 2 for the tail element of
    block 0 (square, add), 9 in block_sum (6 shuffle levels, 3 adds of the wave partials), one per workgroup in the atomicAdd chain onto acc."""
    grid = min(-(-n // (256 * 8 * 4)), 4096)
    chunks = -(-(n // 8) // (grid * 256))
    return 8 * chunks + 2 + 9 + grid


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_adamw_over_bucket_views_matches_clip_grad_norm_and_adamw(cuda, dt):
    """TrainStep.optimizer_step in miniature: six tensors laid flat in one shard at 64-element-aligned offsets (zero padding between them), the
    squared norm by lmx_op_sumsq over the whole shard, then lmx_op_adamw once per bucket view (three views at 64-element boundaries), for three
    steps (clipped, unclipped, clipped).  Reference: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in float64 over the tensors themselves,
    from the state the kernels stored.

    Bound: the one of test_adamw_matches_torch_adamw_in_float64, with the clip factor's relative error widened by half the relative error of the
    fp32 squared norm (gamma_d over the sum of squares, d from _sumsq_depth; the norm itself must be within that).  The padding stays exactly 0."""
    ops = _ops()
    shapes = [(7, 13), (300,), (64, 65), (1000,), (3, 5, 7), (129,)]
    lay, pos = [], 0
    for s in shapes:
        k = int(np.prod(s))
        lay.append((pos, k, s))
        pos += -(-k // 64) * 64
    total = pos
    cuts = [0, lay[2][0], lay[4][0], total]
    pad = torch.ones(total, dtype=torch.bool)
    for o, k, _ in lay:
        pad[o:o + k] = False
    gen = torch.Generator().manual_seed(11)
    master = torch.zeros(total)
    for o, k, _ in lay:
        master[o:o + k] = torch.randn(k, generator=gen) * 0.5
    master = master.to(cuda)
    m = torch.zeros(total, device=cuda)
    v = torch.zeros(total, device=cuda)
    p_shard = torch.empty(total, dtype=dt, device=cuda)
    betas, eps, wd, max_norm = (0.9, 0.999), 1e-8, 0.1, 1.0
    b1, b2, eps32, wd32 = _f32(betas[0]), _f32(betas[1]), _f32(eps), _f32(wd)
    for t, (lr, scale) in enumerate(((1e-2, 3.0), (3e-3, 1e-3), (2e-2, 0.5)), start=1):
        lr32 = _f32(lr)
        g = torch.zeros(total)
        for o, k, _ in lay:
            g[o:o + k] = torch.randn(k, generator=gen) * scale
        g = g.to(dt).to(cuda)
        p0, m0, v0, g64 = (x.double().cpu() for x in (master, m, v, g))
        gsq = torch.zeros(1, dtype=torch.float32, device=cuda)
        ops.sumsq(g, gsq)
        p_shard.fill_(float("nan"))
        for a, b in zip(cuts[:-1], cuts[1:]):
            ops.adamw(p_shard[a:b], g[a:b], master[a:b], m[a:b], v[a:b], lr, betas, eps, wd, t, gnorm_sq=gsq, max_grad_norm=max_norm)
        torch.cuda.synchronize()
        S = float((g64 * g64).sum())
        sq_bound = _gam(_sumsq_depth(total)) * S
        assert abs(gsq.item() - S) <= sq_bound
        ps = [torch.nn.Parameter(p0[o:o + k].view(s).clone()) for o, k, s in lay]
        for p, (o, k, s) in zip(ps, lay):
            p.grad = g64[o:o + k].view(s).clone()
        torch.nn.utils.clip_grad_norm_(ps, max_norm)
        pw, mw, vw = _torch_adamw([p.detach() for p in ps], [p.grad for p in ps], [m0[o:o + k].view(s) for o, k, s in lay],
                                  [v0[o:o + k].view(s) for o, k, s in lay], lr32, (b1, b2), eps32, wd32, t)
        clip = min(1.0, max_norm / (math.sqrt(S) + 1e-6))
        p64, m64, v64, parts = _adamw64(p0, m0, v0, g64, lr32, b1, b2, eps32, wd32, t, clip)
        dclip = sq_bound / S / 2 + 2 * U if clip < 1 else 0.0
        bounds = _adamw_bound(p0, p64, v64, parts, lr32, b1, b2, wd32, t, 5 * U + dclip)
        for (o, k, s), a, b, c in zip(lay, pw, mw, vw):
            for name, x, w, bd in zip(("master", "exp_avg", "exp_avg_sq"), (master, m, v), (a, b, c), bounds):
                r = (x[o:o + k].double().cpu() - w.reshape(-1)).abs() / bd[o:o + k]
                assert r.max().item() <= 1.0, f"step {t}, tensor {s}: {name} is {r.max().item():.3g}x the bound"
        for x in (master, m, v):
            assert (_bits(x.cpu()[pad]) == 0).all()
        assert torch.equal(_bits(p_shard), _bits(master.to(dt)))


# ---- sumsq ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 255 * 8 + 3, 3 * 4096 * 8192 + 13])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_sumsq_accumulates_within_the_summation_bound(cuda, dt, n):
    """lmx_op_sumsq adds sum(x^2) to acc: n below one 8-element chunk (block 0's tail only), one chunk, chunk + tail, 255 chunks + tail, and past
    the 4096-workgroup grid cap (every thread strides over 12 - 13 chunks).  acc starts at 1.5 and the op runs twice; after each call acc must be
    within gamma_d (acc before + sum x^2) of the float64 value, d = _sumsq_depth(n).  |x| >= 0.5, so each element's square is far above that bound
    at the small n and a dropped tail element cannot hide.  All-zero input adds exactly 0."""
    ops = _ops()
    gen = torch.Generator(device=cuda).manual_seed(n % 9973)
    x = torch.randn(n, generator=gen, device=cuda)
    x = (torch.where(x < 0, -0.5, 0.5) + x).to(dt)
    S = float(x.double().square().sum())
    d = _sumsq_depth(n)
    acc = torch.tensor([1.5], dtype=torch.float32, device=cuda)
    ops.sumsq(x, acc)
    assert abs(acc.item() - (1.5 + S)) <= _gam(d) * (1.5 + S)
    ops.sumsq(x, acc)
    assert abs(acc.item() - (1.5 + 2 * S)) <= _gam(d) * (1.5 + S) + _gam(d) * (1.5 + 2 * S)
    del x
    z = torch.zeros(n, dtype=dt, device=cuda)
    for start in (0.0, 1.5):
        acc = torch.tensor([start], dtype=torch.float32, device=cuda)
        ops.sumsq(z, acc)
        assert acc.item() == start


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_sumsq_refuses_a_misaligned_operand(cuda, dt):
    """The kernel reads 8 elements per 16-byte access: an operand one element past an aligned start is refused, and acc is left alone."""
    ops = _ops()
    buf = torch.ones(72, dtype=dt, device=cuda)
    acc = torch.zeros(1, dtype=torch.float32, device=cuda)
    with pytest.raises(_err()):
        ops.sumsq(buf[1:65], acc)
    assert acc.item() == 0.0


# ---- elementwise ------------------------------------------------------------------------------------------------------------------------------
EW_N = [1, 7, 8, 9, 8 * 1000 + 5, 4096 * 11008 + 3]
EW_OFFSETS = [(0, 0, 0), (0, 0, 3), (5, 0, 0), (0, 1, 0), (7, 2, 6)]      # element offsets of a, b, out from 16-byte-aligned starts
SILU_REL = 6 * U          # x / (1 + expf(-x)): expf within 2 ulp (4u), the add and the divide one rounding each
SUB = 2.0 ** -147         # 4 fp32 subnormal spacings: where erfcf's result is subnormal its ulp is absolute


def _silu_bracket(a64, dt):
    """[lo, hi] holding round_T(the kernel's fp32 silu(a)) for any fp32 value within SILU_REL of silu(a): rounding is monotone, so the ends are the
    roundings (through fp32, where the kernel's value lives) of silu(a) (1 -/+ SILU_REL)."""
    s = a64 * torch.sigmoid(a64)
    lo = (s * (1 - SILU_REL)).float().to(dt).double()
    hi = (s * (1 + SILU_REL)).float().to(dt).double()
    return torch.minimum(lo, hi), torch.maximum(lo, hi)


def _inner_rounding_pairs(dt, dev):
    """(a, b) in dt where HF's rounding of silu(a) before the multiply decides the result by a margin fp32 noise cannot blur: silu(a) (1 -/+ SILU_REL)
    round to ONE dt value s_T, and the product without that rounding, round_T(fp32(silu(a) (1 -/+ SILU_REL)) b), is one value other than
    round_T(s_T b)."""
    gen = torch.Generator(device=dev).manual_seed(5)
    a = (torch.randn(1 << 16, generator=gen, device=dev) * 3).to(dt).double()
    b = torch.randn(1 << 16, generator=gen, device=dev).to(dt).double()
    lo, hi = _silu_bracket(a, dt)
    s = a * torch.sigmoid(a)
    n1 = ((s * (1 - SILU_REL)).float().double() * b).float().to(dt).double()
    n2 = ((s * (1 + SILU_REL)).float().double() * b).float().to(dt).double()
    keep = (lo == hi) & (n1 == n2) & (n1 != (lo * b).float().to(dt).double())
    assert int(keep.sum()) >= 128
    return a[keep].to(dt), b[keep].to(dt)


def _ew_inputs(op, dt, n, dev):
    gen = torch.Generator(device=dev).manual_seed(n % 9973 + 17 * op)
    if op == 2:
        a = torch.rand(n, generator=gen, device=dev) * 24 - 12
    else:
        a = torch.randn(n, generator=gen, device=dev) * 3
    b = torch.randn(n, generator=gen, device=dev)
    if op == 3:
        b = b * torch.pow(2.0, torch.randint(-12, 13, (n,), generator=gen, device=dev).float())
    a, b = a.to(dt), b.to(dt)
    if op == 0 and dt != torch.float32:             # the first 64 elements and the last 7 (the scalar tail): pairs where the inner rounding matters
        ca, cb = _inner_rounding_pairs(dt, dev)
        k = min(n, 64)
        a[:k], b[:k] = ca[:k], cb[:k]
        if n > k:
            j = min(7, n - k)
            a[n - j:], b[n - j:] = ca[k:k + j], cb[k:k + j]
    return a, b


def _ew_check(op, dt, a, b, got):
    """Float64 check of one elementwise result (see test_elementwise_paths_agree_and_match_float64)."""
    a64, b64, g64 = a.double(), b.double(), got.double()
    if op == 0:
        lo, hi = _silu_bracket(a64, dt)
        p1, p2 = (lo * b64).float().to(dt).double(), (hi * b64).float().to(dt).double()
        bad = (g64 < torch.minimum(p1, p2)) | (g64 > torch.maximum(p1, p2)) | torch.isnan(g64)
        assert not bad.any(), f"op 0: {int(bad.sum())} outputs are not round(round(silu(a)) * b)"
        return
    if op == 3:
        assert torch.equal(_bits(got), _bits(a + b)), "op 3: not torch's a + b"
        return
    x = a64
    if op == 1:
        ref = 0.5 * x * torch.erfc(-x / math.sqrt(2))
        E = (2 * x * x + 11) * U * ref.abs() + SUB * (x.abs() + 1)
    else:
        P = 0.5 * torch.erfc(-x / math.sqrt(2))
        Q = x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        ref = b64 * (P + Q)
        E = b64.abs() * ((2 * x * x + 10) * U * P + (x * x / 2 + 7) * U * Q.abs() + U * (P + Q).abs() + SUB * (x.abs() + 1)) + U * ref.abs() + SUB
    err = (g64 - ref.float().to(dt).double()).abs()
    bound = _ulp(ref, dt) + E
    bad = ~(err <= bound)
    worst = int((err / bound).nan_to_num(1e30).argmax())
    assert not bad.any(), f"op {op}: {int(bad.sum())} outputs beyond 1 ulp; worst at a = {float(x[worst])}: {float(g64[worst])} vs {float(ref[worst])}"


@pytest.mark.parametrize("n", EW_N)
@pytest.mark.parametrize("op", [0, 1, 2, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_elementwise_paths_agree_and_match_float64(cuda, dt, op, n):
    """lmx_op_elementwise with a, b and out 16-byte aligned (16-bit: the 8-element vector kernel, plus the scalar kernel for the n % 8 tail) and offset
    by 1 - 7 elements each, independently (the scalar kernel throughout).  All placements give the same bits, nothing outside out's window is written,
    and the result matches float64 on the stored inputs:
      op 0, silu(a) * b with HF's rounding points: the kernel's fp32 silu is within 6u of silu(a) (expf 2 ulp, add, divide) and rounding is
        monotone, so the output must lie between round_T(round_T(silu(a) (1 -/+ 6u)) b) — in almost every element one value, bit-exact.  The
        first 64 elements and the last 7 are pairs where dropping the inner rounding gives a value outside that range;
      op 1, gelu_erf(a) = 0.5 a erfc(-a / sqrt2): 1 ulp of T from the once-rounded float64 value, plus the fp32 evaluation error
        (2a^2 + 11) u |gelu|: the rounded argument (constant and product, 2u) moves erfc by its condition number y erfc'(y) / erfc(y) < 2y^2 + 1
        = a^2 + 1 times that, erfcf within 4 ulp (8u), one rounding of the product;
      op 2, b * gelu'(a), |a| <= 12: 1 ulp of T plus |b| ((2a^2 + 10) u P + (a^2 / 2 + 7) u |Q| + u |P + Q|) + u |ref| for
        P = 0.5 erfc(-a / sqrt2) (as in op 1) and Q = a exp(-a^2 / 2) / sqrt(2 pi) (the exponent's rounding moves expf by a^2 / 2 u, expf 2 ulp,
        the constant, two products) — absolute near gelu'(a) = 0 (a ~ -0.75), where the formula itself cancels;
      op 3, a + b: bit-equal to torch's own a + b in T (HF's residual add).
    Where an fp32 intermediate is subnormal (|a| > 13 in op 1) its ulps are absolute: 2^-147 (|a| + 1) more.  For fp32 the 1 ulp is fp32's and
    the evaluation term dominates."""
    ops = _ops()
    a, b = _ew_inputs(op, dt, n, cuda)
    first = None
    for oa, ob, oo in EW_OFFSETS:
        A = torch.empty(n + 16, dtype=dt, device=cuda)
        B = torch.empty(n + 16, dtype=dt, device=cuda)
        O = torch.full((n + 16,), float("nan"), dtype=dt, device=cuda)
        assert (A.data_ptr() | B.data_ptr() | O.data_ptr()) % 16 == 0
        A[oa:oa + n] = a
        B[ob:ob + n] = b
        ops.elementwise(op, A[oa:oa + n], None if op == 1 else B[ob:ob + n], out=O[oo:oo + n])
        got = O[oo:oo + n]
        assert torch.isnan(O[:oo]).all() and torch.isnan(O[oo + n:]).all(), f"offsets {(oa, ob, oo)}: wrote outside out"
        if first is None:
            first = got.clone()
            _ew_check(op, dt, a, b, first)
        else:
            assert torch.equal(_bits(got), _bits(first)), f"offsets {(oa, ob, oo)}: other bits than the aligned call"


# ---- cast_f32 ---------------------------------------------------------------------------------------------------------------------------------
def _midpoints(dt):
    """Every midpoint between two adjacent finite values of the 16-bit dt, both signs (exact in fp32): the round-half-to-even ties, subnormal
    ones included."""
    k = torch.arange(0, (1 << 15) - 1, dtype=torch.int32)
    lo = k.to(torch.int16).view(dt).double()
    hi = (k + 1).to(torch.int16).view(dt).double()
    ok = torch.isfinite(lo) & torch.isfinite(hi)
    mid = ((lo + hi) / 2)[ok]
    return torch.cat([mid, -mid]).float()


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_cast_f32_rounds_like_torch(cuda, dt):
    """lmx_op_cast_f32 (fp32 accumulator -> parameter dtype) against torch.Tensor.to(dt), bit for bit, over +-0, +-inf, NaN, fp32 subnormals, every
    bf16 and f16 rounding tie, the f16 overflow edge (65504, 65519.996, 65520, 65536) and 200001 random fp32 bit patterns.  NaN stays NaN (payloads
    may differ; fp32 -> fp32 keeps every bit).  Odd n: the last workgroup is partial."""
    ops = _ops()
    specials = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 65504.0, 65519.99609375, 65520.0, 65536.0, -65520.0, 1e38,
                             2.0 ** -149, -2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14, 1.0 + 2.0 ** -8,
                             1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], dtype=torch.float32)
    gen = torch.Generator().manual_seed(13)
    rand = torch.randint(-2 ** 31, 2 ** 31, (200001,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    src = torch.cat([specials, _midpoints(torch.bfloat16), _midpoints(torch.float16), rand])
    if src.numel() % 2 == 0:
        src = src[:-1]
    want = src.to(dt)
    out = torch.full((src.numel(),), float("nan"), dtype=dt, device=cuda)
    ops.cast_f32(src.to(cuda), out)
    got = out.cpu()
    if dt == torch.float32:
        assert torch.equal(_bits(got), _bits(src))
        return
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    diff = _bits(got)[~nan] != _bits(want)[~nan]
    assert not diff.any(), f"{int(diff.sum())} values round otherwise than torch, e.g. {src[~nan][diff][:4].tolist()}"


# ---- col_sum ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 255, 257, 4096, 5120])
@pytest.mark.parametrize("rows", [1, 577, 2304, 4097])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_col_sum_within_the_sequential_bound(cuda, dt, rows, cols):
    """lmx_op_col_sum of dy, a column window of a wider buffer (ld = cols + 40, first column 24 elements in): one thread per column adds the rows in
    order in fp32, so each column is within gamma_rows sum_r |dy[r][c]| of the float64 sum (rows - 1 roundings).  Nothing past `cols` is written, and
    a second call gives the same bits (the kernel is deterministic)."""
    ops = _ops()
    gen = torch.Generator(device=cuda).manual_seed(rows * 7 + cols)
    wide = torch.randn((rows, cols + 40), generator=gen, device=cuda).to(dt)
    dy = wide[:, 24:24 + cols]
    out = torch.full((cols + 8,), float("nan"), dtype=torch.float32, device=cuda)
    ops.col_sum(dy, out=out[:cols])
    assert torch.isnan(out[cols:]).all()
    got = out[:cols].double()
    ref = dy.double().sum(0)
    bound = _gam(rows) * dy.double().abs().sum(0)
    assert ((got - ref).abs() <= bound).all(), f"worst {float(((got - ref).abs() / bound).nan_to_num(1e30).max()):.3g}x the bound"
    assert torch.equal(_bits(ops.col_sum(dy)), _bits(out[:cols]))


# ---- gather_embed / embed_bwd -----------------------------------------------------------------------------------------------------------------
EMB_V, EMB_F = 1000, 40


def _embed_plan(dev):
    """Token ids (multiples of 3 only, so the other table rows are never referenced; 0 and V - 1 = 999 among them, id 51 on 1000 more rows), 60 pad
    rows (-1) and the 40 feature rows -2 - k in a random order, all shuffled together."""
    rs = np.random.RandomState(3)
    toks = list(rs.choice(np.arange(0, EMB_V, 3), 1500)) + [0, EMB_V - 1, EMB_V - 1] + [51] * 1000
    src = np.array(toks + [-1] * 60 + list(-2 - rs.permutation(EMB_F)), np.int32)
    rs.shuffle(src)
    return torch.from_numpy(src).to(dev)


@pytest.mark.parametrize("H", [8, 4096, 5120])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_gather_embed_copies_rows_exactly(cuda, dt, H):
    """lmx_op_gather_embed: token rows and feature rows bit-equal to a torch index-gather, pad rows +0 in an output that starts as NaN; a hidden size
    that is not a multiple of 8 is refused."""
    ops = _ops()
    src = _embed_plan(cuda)
    gen = torch.Generator(device=cuda).manual_seed(H)
    table = torch.randn((EMB_V, H), generator=gen, device=cuda).to(dt)
    feats = torch.randn((EMB_F, H), generator=gen, device=cuda).to(dt)
    out = torch.full((src.numel(), H), float("nan"), dtype=dt, device=cuda)
    ops.gather_embed(src, table, feats, out=out)
    s = src.long()
    tok, pad, ft = s >= 0, s == -1, s <= -2
    assert torch.equal(_bits(out[tok]), _bits(table[s[tok]]))
    assert torch.equal(_bits(out[ft]), _bits(feats[-2 - s[ft]]))
    assert (_bits(out[pad]) == 0).all()
    with pytest.raises(_err()):
        ops.gather_embed(src, torch.zeros((EMB_V, 12), dtype=dt, device=cuda), torch.zeros((EMB_F, 12), dtype=dt, device=cuda))


@pytest.mark.parametrize("H", [8, 4096, 5120])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_embed_bwd_scatter_adds_within_the_atomics_bound(cuda, dt, H):
    """lmx_op_embed_bwd on the plan of test_gather_embed_copies_rows_exactly.  The fp32 table gradient is a float64 scatter-add of the token rows'
    gradients up to the order of the atomics: row id is within count(id) u sum |d| of it, per column (count(id) fp32 adds onto 0, in any order).
    Table rows no token refers to stay exactly +0; pad rows carry gradients of 1e3, which must reach nothing.  The feature rows' gradients land
    bit-equal in dfeats (NaN beforehand).  dtable32=None and dfeats=None each give the other output alone, the same."""
    ops = _ops()
    src = _embed_plan(cuda)
    s = src.long()
    tok, pad, ft = s >= 0, s == -1, s <= -2
    gen = torch.Generator(device=cuda).manual_seed(H + 1)
    d = torch.randn((src.numel(), H), generator=gen, device=cuda).to(dt)
    d[pad] = 1e3
    dtable = torch.zeros((EMB_V, H), dtype=torch.float32, device=cuda)
    dfeats = torch.full((EMB_F, H), float("nan"), dtype=dt, device=cuda)
    ops.embed_bwd(src, d, dtable, dfeats)
    ref = torch.zeros((EMB_V, H), dtype=torch.float64, device=cuda).index_add_(0, s[tok], d[tok].double())
    mag = torch.zeros((EMB_V, H), dtype=torch.float64, device=cuda).index_add_(0, s[tok], d[tok].double().abs())
    cnt = torch.bincount(s[tok], minlength=EMB_V).double()
    bound = cnt[:, None] * U * mag

    def check_table(t):
        over = (t.double() - ref).abs() - bound
        assert (over <= 0).all(), f"{int((over > 0).sum())} entries past the bound"
        assert (_bits(t[cnt == 0]) == 0).all()

    check_table(dtable)
    assert torch.equal(_bits(dfeats[-2 - s[ft]]), _bits(d[ft]))
    t2 = torch.zeros_like(dtable)
    ops.embed_bwd(src, d, t2, None)
    check_table(t2)
    f2 = torch.full_like(dfeats, float("nan"))
    ops.embed_bwd(src, d, None, f2)
    assert torch.equal(_bits(f2), _bits(dfeats))
