"""float64 statements of the non-linear half of the forward path — RoPE with the KV append, RMSNorm, LayerNorm and the attention family — with per-element error
bounds that are DERIVED from the kernels' arithmetic as read in csrc/ (common.h, elementwise.hip, attention.hip, attention_decode.h, attention_batch.h,
decode_attn.hip), never fitted to their output.  Conventions of linear_ref.py, whose U / rnd / check / norm_chain / FLIP_MAX_FRACTION and ulp helpers are used as they
are.  Shared by test_forward_ref_host.py (which proves on the CPU that honest emulations of the kernels' arithmetic stay inside every bound and that subtly wrong
arithmetic falls outside) and test_forward_fp64_gpu.py / the tightened assertions of the older GPU tests.

Inputs of the shared cases are drawn HERE, on the CPU with fixed seeds, so the host proof and the GPU run see the same numbers.

One fp32 operation (add, mul, fma, correctly rounded division) moves its result by at most U |result|, U = 2^-24.  v_exp_f32 / v_log_f32 (exp2 / log2) are taken at
the HIP math API reference's 1 ulp = 2 U relative, as linear_ref.act64 takes the exponential; rsqrtf at that reference's 1 ulp = 2 U."""
import math

import torch

from linear_ref import DT, FLIP_MAX_FRACTION, U, check, norm_chain, rnd, ulp_of  # noqa: F401  (re-exported)

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
UT = {"bf16": 2.0 ** -9, "f16": 2.0 ** -12}       # unit roundoff of the 16-bit storage types (8 / 11 significand bits)
SECOND_ORDER = 1 + 2.0 ** -10                     # first-order perturbation terms are below 1e-4 here: their squares are below 2^-10 of them
FA_DEFER = 8.0                                    # attention_mfma.h: the prefill kernel's running max may lag the true one by 2^8


def gen(seed):
    return torch.Generator().manual_seed(seed)


# =====================================================================================================================================================================
# RoPE
# =====================================================================================================================================================================
ROPE_DTYPES = ("bf16", "f16", "f32")
ROPE_GEOMS = ((128, 4, 4), (64, 4, 2), (128, 8, 2))      # (D, nh, nkv)
ROPE_T = (1, 63, 64, 65, 150)                            # the grid is ceil(T / 64)
ROPE_S_MAX = 256


def rope_pos0(T, s_max=ROPE_S_MAX):
    return (0, 37, s_max - T)


def rope_table(n_pos, D, theta=10000.0):
    """[n_pos, D] float32: cos half | sin half (what the engine uploads)."""
    inv = 1.0 / (theta ** (torch.arange(0, D, 2).float() / D))
    fr = torch.arange(n_pos).float()[:, None] * inv[None, :]
    return torch.cat([fr.cos(), fr.sin()], dim=-1).contiguous()


def rope_chain(x, pos, table, dt):
    """HF's chain T( T(x c) + T(rot(x) s) ) of x [T, heads, D] (stored dtype) at positions pos [T], evaluated EXACTLY; returns (ref64, E).

    cos / sin are rounded to T first (round_to<T>(cs[..]) in every kernel).  16-bit T: x c and r s are products of two T values (16 / 22 significand bits), exact in
    float64; p + q of two T values is exact in float64 unless their exponents are more than 40 binades apart, and then the sum is within 2^-40 of p, nowhere near a
    rounding boundary of T — so every rnd() below rounds the exact value once and the statement is BIT EQUALITY: E is None.
    T = float: rope_term (contraction off) is fl(fl(x c) + fl(r s)).  |fl(x c) - x c| <= U |x c|, likewise r s; the add rounds once more, U |p + q| <=
    U (1 + U) (|x c| + |r s|):   E = (2 U + U^2) (|x c| + |r s|),   and check() adds ulp_T(ref) on top."""
    D = x.shape[-1]
    tb = table.to(x.device).to(DT[dt]).double()
    c = torch.cat([tb[pos, : D // 2]] * 2, -1)[:, None, :]
    s = torch.cat([tb[pos, D // 2:]] * 2, -1)[:, None, :]
    xd = x.double()
    rot = torch.cat([-xd[..., D // 2:], xd[..., : D // 2]], -1)
    if dt == "f32":
        return xd * c + rot * s, (2 * U + U * U) * ((xd * c).abs() + (rot * s).abs())
    return rnd(rnd(xd * c, dt) + rnd(rot * s, dt), dt), None


def exact_equal(got, ref64, what=""):
    """Bit equality of a 16-bit result with a float64 statement that is itself a value of T (-0 == +0)."""
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    bad = got.double() != ref64
    n_bad = int(bad.sum())
    if n_bad:
        i = int(bad.flatten().double().argmax())
        raise AssertionError(f"{what}: {n_bad} of {bad.numel()} elements differ from the exact chain; first at flat index {i}: "
                             f"got {float(got.flatten()[i])!r}, chain {float(ref64.flatten()[i])!r}")


def rope_check(got, x, pos, table, dt, what=""):
    """got [T, heads, D] against the chain of x: bit equality for 16-bit types, the derived bound for float.  Returns the worst err / bound (0 for equality)."""
    ref, E = rope_chain(x, pos, table, dt)
    if E is None:
        exact_equal(got, ref, what)
        return 0.0
    return check(got, ref, E, dt, what)


def rope_inputs(D, nh, nkv, T, dt, seed=1):
    return torch.randn(T, (nh + 2 * nkv) * D, generator=gen(seed + 7 * T + D)).to(DT[dt])


# =====================================================================================================================================================================
# norms
# =====================================================================================================================================================================
RMS_H = (8, 264, 1024, 4096, 5120, 8192, 8200)    # rmsnorm_reg_kernel<T, 1> with idle threads (8, 264), <1> <2> <3> <4> full, rmsnorm_kernel (H > 8192)
LN_H = (512, 1024, 2048, 1536, 1032, 4096)        # layernorm_wave_kernel<T, 1 | 2 | 4>, the generic kernel (1536, not a multiple of 512, > 2048)
NORM_ROWS = (1, 5, 70)                            # 5 % 4 != 0: the wave kernel's row tail
NORM_EPS = 1e-5


def norm_inputs(rows, H, dt, seed=0):
    """(x [rows + 2, H], w, b) in T: randn * 3 + 0.5 rows, then an OFFSET row 100 + 0.01 randn and a CONSTANT row (zero variance).  For 16-bit T the seed is advanced
    until the RMSNorm flippable set of x stays under FLIP_MAX_FRACTION of a row (at H = 8 a single flippable element is 12.5 % of the row): a property of the
    float64 reference alone, found without any kernel."""
    for s in range(seed, seed + 64):
        g = gen(1000 * s + 13 * rows + H)
        x = torch.randn(rows, H, generator=g) * 3 + 0.5
        off = 100 + 0.01 * torch.randn(1, H, generator=g)
        x = torch.cat([x, off, torch.full((1, H), 2.5)], 0).to(DT[dt])
        w = (1 + 0.1 * torch.randn(H, generator=g)).to(DT[dt])
        b = (0.1 * torch.randn(H, generator=g)).to(DT[dt])
        if float(norm_chain(x, dt, NORM_EPS)[1].double().mean(-1).max()) <= FLIP_MAX_FRACTION:
            return x, w, b
    raise AssertionError("no seed keeps the flippable set under the cap")


def _sum_units(H):
    """Roundings on a row sum of H terms: a thread adds 8 elements per 2048 columns in sequence, wave_sum adds 6 levels, block_sum the 4 waves (3 non-trivial adds);
    the one-wave LayerNorm kernel adds 8, 6 levels, then its H / 512 <= 4 chunk sums: 18 at most.  8 ceil(H / 2048) + 10 covers both."""
    return 8 * ((H + 2047) // 2048) + 10


def rmsnorm_ref(x, w, dt, eps=NORM_EPS):
    """(ref64, flip, E) of   y = round_T( round_T(x inv) w ),   inv = rsqrt(mean(x^2) + eps) with fp32 statistics.

    16-bit T: x * inv is one fp32 product rounded to T at once, and round_T(x inv) * w is exact in fp32 (8 + 8 / 11 + 11 significand bits) before its rounding
    to T, so the kernel's value differs from the float64 chain ONLY where x inv sits so close to a rounding boundary of T that the kernel's fp32 inv puts it on the other side: norm_chain's flippable set.
    Outside it: equality (E = 0).  Inside: one ulp_T of the first rounding carried through w, and the second rounding may land one ulp_T(ref) away:
        E = flip (ulp_T(x inv) |w| + ulp_T(ref)).
    T = float: ss is a sum of H positive fmaf terms, _sum_units(H) roundings, then / H and + eps (2 more): relative (_sum_units + 2) U, halved by the square root;
    rsqrtf 2 U; x * inv and * w one rounding each:   E = ((_sum_units(H) + 2) / 2 + 4) U |ref|."""
    p, flip = norm_chain(x, dt, eps)
    wd = w.double()
    if dt == "f32":
        ref = p * wd
        return ref, flip, ((_sum_units(x.shape[-1]) + 2) / 2 + 4) * U * ref.abs()
    ref = rnd(rnd(p, dt) * wd, dt)
    return ref, flip, flip.double() * (ulp_of(p, dt) * wd.abs() + ulp_of(ref, dt))


def rmsnorm_check(got, x, w, dt, eps=NORM_EPS, what=""):
    """Asserts the cap on the flippable set, then the statement above at every element.  Returns (worst err / bound for float | share of elements that differ from the
    chain for 16-bit, the largest flippable share of a row)."""
    ref, flip, E = rmsnorm_ref(x, w, dt, eps)
    frac = float(flip.double().mean(-1).max())
    assert frac <= FLIP_MAX_FRACTION, f"{what}: flippable fraction {frac:.4f} of a row: choose other inputs"
    if dt == "f32":
        return check(got, ref, E, dt, what), frac
    assert got.shape == ref.shape and torch.isfinite(got.float()).all(), f"{what}: shape / non-finite outputs"
    err = (got.double() - ref).abs()
    bad = err > E
    n_bad = int(bad.sum())
    if n_bad:
        i = int((err - E).flatten().argmax())
        raise AssertionError(f"{what}: {n_bad} of {err.numel()} outputs off the chain round_T(round_T(x inv) w) ({int((bad & ~flip).sum())} outside the flippable set); "
                             f"worst at flat index {i}: got {float(got.flatten()[i])!r}, chain {float(ref.flatten()[i])!r}, allowed {float(E.flatten()[i]):.3e}")
    return float((err > 0).double().mean()), frac


def layernorm_ref(x, w, b, dt, eps=NORM_EPS):
    """(ref64, E) of the kernels' two-pass chain   y = round_T( (x - mean) rstd w + b ),   mean, rstd from fp32 statistics; check() adds the final ulp_T(ref).

    With c = _sum_units(H), d = x - mean, var = mean(d^2), mad = mean |d|, r = rsqrt(var + eps):
      * mean = fl(sum) / H:  c roundings on the sum, one for the division:            dm = (c + 1) U mean|x|
      * d_k = fl(x - mean_k): off by dm, rounded once:                                 dd = dm + U |d|
      * q = sum d_k^2 (fmaf), / H, + eps: the shift dm moves var by 2 dm mad + dm^2, the roundings of d by 2 U var, sum / division / add by (c + 2) U (var + eps):
                                                                                       rel_v = (2 dm mad + dm^2) / (var + eps) + (c + 4) U
      * rstd = rsqrtf(var + eps): half of rel_v, plus rsqrtf's documented 1 ulp:       rel_r = rel_v / 2 + 2 U
      * d * rstd, * w: one rounding each; + b (an fma or an add): one rounding of y:
            E = r |w| dd + |d r w| (rel_r + 2 U) + U |ref|.
    On the constant row var = 0 and r = eps^-1/2 = 316: whatever the row sum loses (dm) is amplified by r |w| — the bound says so, it is not an allowance."""
    xd, wd, bd = x.double(), w.double(), b.double()
    H = x.shape[-1]
    c = _sum_units(H)
    e32 = float(torch.tensor(eps, dtype=torch.float32))
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    var = d.pow(2).mean(-1, keepdim=True)
    mad = d.abs().mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + e32)
    ref = d * r * wd + bd
    dm = (c + 1) * U * xd.abs().mean(-1, keepdim=True)
    dd = dm + U * d.abs()
    rel_v = (2 * dm * mad + dm * dm) / (var + e32) + (c + 4) * U
    rel_r = rel_v / 2 + 2 * U
    E = r * wd.abs() * dd + (d * r * wd).abs() * (rel_r + 2 * U) + U * ref.abs()
    return ref, E * SECOND_ORDER


def layernorm_check(got, x, w, b, dt, eps=NORM_EPS, what=""):
    ref, E = layernorm_ref(x, w, b, dt, eps)
    return check(got, ref, E, dt, what)


# =====================================================================================================================================================================
# attention
# =====================================================================================================================================================================
PREFILL_DTYPES = ("bf16", "f16")
PREFILL_CASES = ((128, 4, 4, 330, 0, True), (128, 4, 2, 200, 300, True), (128, 2, 2, 1, 77, True), (128, 2, 2, 64, 0, True),      # (D, nh, nkv, Tq, past, causal)
                 (64, 4, 4, 577, 0, False), (64, 2, 1, 130, 0, True), (64, 2, 2, 50, 0, False))
DECODE_DTYPES = ("bf16", "f16", "f32")
DECODE_CASES = ((128, 4, 4, 1, 1100, True, 8), (128, 4, 2, 1, 5, True, 8), (128, 2, 2, 40, 30, True, 1), (64, 4, 4, 33, 0, False, 1),   # (D, nh, nkv, rows, past, causal, n_split)
                (64, 2, 1, 1, 700, True, 4))
DECODE_NONCAUSAL_KEYS = 577
STEP_GEOMS = ((4, 4, 128), (8, 2, 128), (4, 4, 64))      # (nh, nkv, D)
STEP_POS = (0, 1, 127, 128, 129, 300)
STEP_S_MAX = 512


def attn_inputs(D, nh, nkv, Tq, Tk, dt, seed, flat=False):
    """q [Tq, nh, D], k / v [Tk, nkv, D] in T: randn; flat: k scaled by 0.05, so every p is about 1 / Tk — each key carries little weight and a max-norm is blindest."""
    g = gen(seed)
    q = torch.randn(Tq, nh, D, generator=g); k = torch.randn(Tk, nkv, D, generator=g); v = torch.randn(Tk, nkv, D, generator=g)
    if flat:
        k = k * 0.05
    return q.to(DT[dt]), k.to(DT[dt]), v.to(DT[dt])


def forced_rescale_inputs(dt="bf16"):
    """test_flash_attn_forced_rescale's input: a late key with a huge score forces the online-softmax rescale branch.  (D, nh, nkv, Tq, past, causal) = (128, 2, 2, 256, 0, T)."""
    g = gen(0)
    D, nh, Tq = 128, 2, 256
    q = torch.randn(Tq, nh, D, generator=g); k = torch.randn(Tq, nh, D, generator=g) * 0.1; v = torch.randn(Tq, nh, D, generator=g)
    k[200] = q[220] * 4.0
    return q.to(DT[dt]), k.to(DT[dt]), v.to(DT[dt])


def step_inputs(nh, nkv, D, pos, dt, seed=0, flat=False):
    """(qkv row [(nh + 2 nkv) D] pre-RoPE, k_past, v_past [pos, nkv, D]) of one decode step."""
    g = gen(seed + 31 * pos + nh + D)
    row = torch.randn((nh + 2 * nkv) * D, generator=g)
    k_past = torch.randn(pos, nkv, D, generator=g) * (0.05 if flat else 1.0)
    v_past = torch.randn(pos, nkv, D, generator=g)
    if flat:
        row[nh * D:(nh + nkv) * D] *= 0.05
    return row.to(DT[dt]), k_past.to(DT[dt]), v_past.to(DT[dt])


class AttnRef:
    """Exact softmax(q k^T / sqrt D) v in float64 on the stored inputs.  q [Tq, nh, D], k / v [Tk, nkv, D]; causal: row i sees keys 0 .. q_pos0 + i.
        ref [Tq, nh, D]      the output
        mag [Tq, nh, D]      sum_j p_ij |v_jd|
        lse2 [nh, Tq]        log2 sum_j 2^(s_ij): the log-sum-exp of the scaled scores in the log2 domain (what the prefill kernel's lse output holds)
        P, S, A [nh, Tq, Tk] probabilities, log2-domain scores (-inf where masked), and sum_e |q_e k_je| scale log2(e): what a dot product's roundings are relative to
    dq / dk (optional, same shapes as q / k): absolute error bounds of the kernel's own q / k where it computes them in fp32 (RoPE of float models)."""

    def __init__(self, q, k, v, causal, q_pos0, dq=None, dk=None):
        Tq, nh, D = q.shape
        Tk, nkv, _ = k.shape
        self.D, self.Tk = D, Tk
        rep = nh // nkv
        qd = q.double()
        kd = k.double().repeat_interleave(rep, dim=1)
        self.vd = v.double().repeat_interleave(rep, dim=1)
        sc = LOG2E / math.sqrt(D)
        S = torch.einsum("qhd,khd->hqk", qd, kd) * sc
        self.A = torch.einsum("qhd,khd->hqk", qd.abs(), kd.abs()) * sc
        self.dS = None
        if dq is not None or dk is not None:
            z = torch.zeros_like(self.A)
            self.dS = (z if dq is None else torch.einsum("qhd,khd->hqk", dq.double(), kd.abs()) * sc) + \
                      (z if dk is None else torch.einsum("qhd,khd->hqk", qd.abs(), dk.double().repeat_interleave(rep, dim=1)) * sc)
        self.visible = torch.ones(Tq, Tk, dtype=torch.bool, device=q.device)
        if causal:
            self.visible = torch.arange(Tk, device=q.device)[None, :] <= torch.arange(Tq, device=q.device)[:, None] + q_pos0
        S = S.masked_fill(~self.visible[None], float("-inf"))
        self.M = S.max(-1, keepdim=True).values
        w = torch.exp2(S - self.M)
        l = w.sum(-1, keepdim=True)
        self.S, self.P = S, w / l
        self.lse2 = (self.M + torch.log2(l)).squeeze(-1)
        self.ref = torch.einsum("hqk,khd->qhd", self.P, self.vd)
        self.mag = torch.einsum("hqk,khd->qhd", self.P, self.vd.abs())
        self.n_keys = self.visible.sum(-1)                                                       # [Tq]

    def _weight_eps(self, dot_units, n_exp, lag=0.0):
        """Relative error bound of every key's weight 2^(s_j - M) as the kernels form it, [nh, Tq, Tk] (0 where masked):
          * the score: dot_units roundings relative to A_j (the fmaf chain / MFMA accumulation and the shuffle tree), the constant scale log2(e) formed in fp32 from
            the float scale (3 U) and the product with it (1 U) relative to |s_j| <= A_j: (dot_units + 4) U A_j in the log2 domain, ln 2 times that on the weight;
            plus ln 2 dS where the kernel's own q / k carry an error;
          * every subtraction in front of an exp2 rounds once, U |s - m|; along a key's path (its chunk's max, the merge max, the newest key's max) the arguments
            add up to M - s_j (+ `lag` where a running max may lag): ln 2 U (M - s_j + lag);
          * n_exp evaluations of v_exp_f32 multiply into the weight: 2 U each."""
        gap = torch.where(torch.isfinite(self.S), self.M - self.S + lag, torch.zeros_like(self.S))
        e = LN2 * ((dot_units + 4) * U * self.A + U * gap) + 2 * U * n_exp
        if self.dS is not None:
            e = e + LN2 * self.dS
        return torch.where(torch.isfinite(self.S), e, torch.zeros_like(e))

    def fp32_bound(self, dot_units, pv_units, sum_units, merge_units, n_exp, lag=0.0):
        """E [Tq, nh, D] for a kernel that keeps P in fp32:   |got - round_T(ref)| <= ulp_T(ref) + E.

        out = sum_j w_j v_j / sum_j w_j.  A relative error e_j on w_j moves out by sum_j p_j e_j (v_j - out) to first order (the common part of the e_j cancels
        between numerator and denominator), SECOND_ORDER covers the rest:     sum_j p_j e_j |v_jd - out_d|.
        The sums themselves: numerator pv_units (fmaf chain + shuffle tree of P V inside a chunk) + merge_units (weighting and adding the chunk partials, the newest
        key's fold) roundings relative to mag; denominator sum_units + merge_units relative to 1, carried to the output through |out| <= mag; the division 3 U as in
        linear_ref.  An addition of an exact zero does not round, so a chain over n keys rounds at most n times: pv_units and sum_units are capped by the row's key
        count.  Results of v_exp_f32 below the smallest normal may be flushed: 2^-126 sum_j |v_jd|."""
        eps = self._weight_eps(dot_units, n_exp, lag)
        W = self.P * eps
        nk = self.n_keys.double()[:, None, None]
        units = torch.clamp(nk, max=pv_units) + torch.clamp(nk, max=sum_units) + 2 * merge_units + 3
        flush = 2.0 ** -126 * torch.einsum("qk,khd->qhd", self.visible.double(), self.vd.abs())
        return SECOND_ORDER * self._dev(W) + units * U * self.mag + flush

    def _dev(self, W):
        """sum_j W_j |v_jd - out_d|, [Tq, nh, D], without materialising [nh, Tq, Tk, D]: by key blocks."""
        out = torch.zeros_like(self.ref)
        for k0 in range(0, self.Tk, 64):
            dv = (self.vd[None, k0:k0 + 64] - self.ref[:, None]).abs()                           # [Tq, kb, nh, D]
            out += torch.einsum("hqk,qkhd->qhd", W[:, :, k0:k0 + 64], dv)
        return out

    # ---- the kernels --------------------------------------------------------------------------------------------------------------------------------------
    def _dot_units(self):
        return 8 + int(math.log2(self.D // 8))                    # 8 fmaf per lane, then a butterfly over the D / 8 lanes of a key

    def decode_attn_bound(self, n_split):
        """decode_attn_kernel + decode_attn_combine_kernel (attention.hip).  A split holds ceil(ceil(n / n_split) / 64) 64 keys: P V is one fmaf chain of 8 per 64
        keys and 3 shuffle adds; the sum adds ceil(chunk / 256) per thread, 6 levels, 3 waves; the combine weighs and adds n_split partials (2 n_split roundings);
        two exp2 per weight (p, the split's weight)."""
        chunk = (((self.Tk + n_split - 1) // n_split + 63) // 64) * 64
        return self.fp32_bound(self._dot_units(), chunk // 8 + 3, (chunk + 255) // 256 + 9, 2 * n_split, 2)

    def step_bound(self, n_split):
        """dec_attn_chunk (decode_attn.hip) and decode_fused_body (attention_decode.h): 128-key chunks, P V 16 fmaf + 3 shuffle adds, the sum 6 levels + 3 waves,
        the merge one product and at most n_split adds per partial, then the newest key's fold (a product and an fma) — n_split + 3; three exp2 per weight (p, the
        chunk's weight, the fold's).  decode_fused_body folds the newest key inside its chunk instead: fewer roundings, same bound."""
        return self.fp32_bound(self._dot_units(), 19, 9, n_split + 3, 3)

    def batch_wave_bound(self, n_waves=4):
        """decode_attn_wave_kernel (attention_batch.h): a wave walks ppw = ceil(pieces / n_waves) 64-key pieces online: per piece the accumulator is rescaled (1)
        and takes 8 fmaf, 3 shuffle adds at the end; l takes a product, 6 levels and an add per piece; the merge weighs and adds n_waves + 1 states; a weight sees
        its own exp2, up to ppw rescales and the merge's."""
        ppw = max(1, ((self.Tk - 1 + 63) // 64 + n_waves - 1) // n_waves)
        return self.fp32_bound(self._dot_units(), 9 * ppw + 3, 8 * ppw, 2 * (n_waves + 1), ppw + 2)

    def prefill_bound(self, dt):
        """flash_prefill2_kernel (attention.hip): P is rounded to T as the MFMA operand, relative u_T per probability; l is summed from the unrounded values:
        u_T mag.  A second u_T mag holds everything fp32 does (prefill_fp32_part, asserted to fit by test_forward_ref_host.py for every input the GPU test uses):
            E = 2 u_T mag,   and check() adds ulp_T(ref).   For bf16 this is the bound of test_flash_attn_real_shape_vs_fp32_and_hf_rounding_chain."""
        return 2 * UT[dt] * self.mag

    def _prefill_counts(self):
        tiles = (self.Tk + 63) // 64
        return tiles, (tiles + 1) // 2                             # key tiles, tiles per wave group

    def prefill_fp32_part(self, dt):
        """What the prefill kernel's fp32 arithmetic adds, to be held under u_T mag: the MFMA dot product over D terms (D roundings at most, whatever the order
        inside the instruction), P V accumulated over the 64 keys of a tile and a rescale per tile, for the tiles of one wave group; l: 32 adds per tile, the tile's
        add and rescale; merge of the two groups and the two lane halves (4); a weight sees its own exp2, a rescale per tile and the merge's; the running max may
        lag by 2^FA_DEFER.  f16 only: a P below 2^-14 is subnormal in T, absolute error 2^-25 at most and never more than the value itself (it rounds to 0 at
        worst), on a weight scale where l >= 1 (the key that set the running max has weight >= 1):  sum_j min(2^-25, p_j) |v_jd|."""
        tiles, tpg = self._prefill_counts()
        E = self.fp32_bound(self.D, 65 * tpg, 34 * tpg, 4, tpg + 2, lag=FA_DEFER)
        if dt == "f16":
            E = E + torch.einsum("hqk,khd->qhd", self.P.clamp(max=2.0 ** -25), self.vd.abs())
        return E

    def lse_bound(self):
        """E [nh, Tq] of the prefill kernel's lse = m + log2(l) against lse2, both fp32 / float64 in the log2 domain:
          * the scores: a shift ds_j of every s_j moves lse2 by at most sum_j p_j ds_j,  ds_j = (D + 4) U A_j  (MFMA dot product over D terms, the scale constant
            and the product with it);
          * l: relative error  2 U n_exp + ln 2 U sum_j p_j (M - s_j + FA_DEFER) + chain U  with n_exp = tiles per group + 2 and chain = 34 tiles per group + 4 as in
            prefill_fp32_part; 1 / ln 2 of it in the log2 domain;
          * v_log_f32: 1 ulp of its result, |log2 l| <= log2(keys) + FA_DEFER:  2 U (log2 Tk + FA_DEFER + 1);
          * the add m + log2 l: U |lse2|."""
        tiles, tpg = self._prefill_counts()
        gap = torch.where(torch.isfinite(self.S), self.M - self.S + FA_DEFER, torch.zeros_like(self.S))
        rel_l = 2 * U * (tpg + 2) + LN2 * U * (self.P * gap).sum(-1) + (34 * tpg + 4) * U
        return (self.P * (self.D + 4) * U * self.A).sum(-1) + rel_l / LN2 + 2 * U * (math.log2(max(self.Tk, 2)) + FA_DEFER + 1) + U * self.lse2.abs()


def step_ref(row, k_past, v_past, table, pos, nh, nkv, D, dt):
    """One decode step in float64: RoPE of q and the new key at `pos` by the exact chain, append, attention of the one query over keys 0 .. pos.
    Returns (AttnRef, k_new64 [nkv, D], kE or None, v_new [nkv, D]).  For float the kernel's rotated q / k_new carry rope_chain's E, handed to AttnRef as dq / dk."""
    p1 = torch.tensor([pos], device=row.device)
    q_r, qE = rope_chain(row[: nh * D].view(1, nh, D), p1, table, dt)
    k_r, kE = rope_chain(row[nh * D:(nh + nkv) * D].view(1, nkv, D), p1, table, dt)
    v_n = row[(nh + nkv) * D:].view(1, nkv, D)
    k_all = torch.cat([k_past.double(), k_r], 0); v_all = torch.cat([v_past, v_n], 0)
    dk = None
    if kE is not None:
        dk = torch.cat([torch.zeros_like(k_past, dtype=torch.float64), kE], 0)                    # E bounds |kernel's value - exact| by itself
    return AttnRef(q_r, k_all, v_all, False, 0, dq=qE, dk=dk), k_r[0], (kE[0] if kE is not None else None), v_n[0]


def append_check(k_row, k_new64, kE, dt, what=""):
    """The appended K row [nkv, D]: bit-equal to the chain for 16-bit types, inside the derived bound for float."""
    if kE is None:
        exact_equal(k_row, k_new64, what)
        return 0.0
    return check(k_row, k_new64, kE, dt, what)
