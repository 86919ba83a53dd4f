"""Shared fixture of the cache-tail tests: one layer's K / V^T caches with valid keys in [0, n) and a tail [n, s_max) in one of three states, and output
buffers set inside NaN-filled sentinel space.

A recycled engine sequence (lmx_seq_create takes it from the pool), a truncated one (lmx_seq_truncate) and the training step's per-length scratch pairs
keep whatever earlier work left past the valid length.  Nothing stored there may reach an output: the kernels mask by length.  The tail states are the
ones of test_decode_batch_attn_gpu._build:
    zero       what ops.alloc_kv hands out (hides any read of V past the length: such a read adds nothing)
    stale      finite values of an earlier request, randn * 50
    nonfinite  K = NaN, V^T = Inf with NaN on every third slot (0 x Inf = NaN: a masked key's V must not even be multiplied by its zero probability)
Not a conftest: imported by the tests that use it."""
import torch

from test_ops_gpu import DT, TOL, _attn_ref, _fill_cache, _rel_err, _rope_ref, _rope_table  # noqa: F401  (re-exported for the tests)

TAILS = ("zero", "stale", "nonfinite")


def poison_tail(kc, vt, n, tail, seed=0):
    """Overwrite slots [n, s_max) of kc [nkv, s_max, D] / vt [nkv, D, s_max] with the tail state `tail` (own generator: the valid keys do not depend on it)."""
    nkv, s_max, D = kc.shape
    if n >= s_max:
        return
    if tail == "zero":
        kc[:, n:] = 0
        vt[:, :, n:] = 0
    elif tail == "stale":
        g = torch.Generator(device=kc.device).manual_seed(7919 + seed)
        kc[:, n:] = (torch.randn(nkv, s_max - n, D, device=kc.device, generator=g) * 50).to(kc.dtype)
        vt[:, :, n:] = (torch.randn(nkv, D, s_max - n, device=kc.device, generator=g) * 50).to(vt.dtype)
    elif tail == "nonfinite":
        kc[:, n:] = float("nan")
        vt[:, :, n:] = float("inf")
        vt[:, :, n::3] = float("nan")
    else:
        raise ValueError(tail)


def tail_caches(k, v, s_max, dtype, tail, seed=0):
    """Caches holding k / v [n, nkv, D] in slots [0, n) and the tail state `tail` behind them."""
    kc, vt = _fill_cache(k, v, s_max, dtype, k.device)
    poison_tail(kc, vt, k.shape[0], tail, seed)
    return kc, vt


def bits(t):
    """Integer view of the same bytes: NaN == NaN, -0 != +0."""
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


class Window:
    """A [rows, cols] output that is a window of a NaN-filled buffer: `pad` sentinel rows above and below, `pad_c` sentinel columns either side (8: the
    window's rows keep 16-byte alignment).  `out` is the window (row stride cols + 2 pad_c); `row` is its single row when rows == 1 (contiguous)."""

    def __init__(self, rows, cols, dtype, device, pad=2, pad_c=8):
        self.big = torch.full((rows + 2 * pad, cols + 2 * pad_c), float("nan"), dtype=dtype, device=device)
        self.sl = (slice(pad, pad + rows), slice(pad_c, pad_c + cols))
        self.out = self.big[self.sl]
        self.row = self.out[0] if rows == 1 else None
        self.before = self.big.clone()

    def untouched_outside(self):
        after = self.big.clone()
        after[self.sl] = self.before[self.sl]
        return same_bits(after, self.before)


def caches_kept(kc, vt, before, appended=None):
    """Every byte of both caches as in `before` (prefix AND tail), except slot `appended` (the key / value a decode launch appends)."""
    kb, vb = before
    if appended is None:
        return same_bits(kc, kb) and same_bits(vt, vb)
    keep = torch.ones(kc.shape[1], dtype=torch.bool, device=kc.device)
    keep[appended] = False
    return same_bits(kc[:, keep], kb[:, keep]) and same_bits(vt[:, :, keep], vb[:, :, keep])
