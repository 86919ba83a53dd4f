"""The LoRA dropout mask in numpy: the restatement of csrc/dropout.h that a reference (or a test) reproduces a training step with.

peft gives every adapted linear its own nn.Dropout, y = base(x) + scaling * lora_B(lora_A(dropout(x))); the reference's LoRA scripts run it at p = 0.05
(llava/train/train.py:113, :879).  Here the mask is a pure function of a counter, so the forward, a recomputed layer and the backward kernels regenerate it:

    generator   Philox4x32-10 (Random123's philox4x32_10)
    one call    per aligned group of 8 columns: counter = (row, col >> 3, stream, step), key = the 64-bit seed split (lo, hi)
    stream      rank << 16 | layer << 3 | index of the module in train.LORA_MODULES
    keep rule   the four output words are eight 16-bit lanes; column c takes word (c & 7) >> 1, the low half for even c; keep iff lane >= thr

thr = round(p * 65536): the drop probability is p ROUNDED TO A MULTIPLE OF 2^-16 (0.05 -> 3277 / 65536 = 0.0500031).  Kept values are scaled by
fp32(1 / (1 - p)) of the p that was asked for, and rounded once to the tensor's dtype; dropped ones are +0."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def _check_p(p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must be in [0, 1) (got {p})")
    return p


def threshold(p: float) -> int:
    """thr of the keep rule: round(p * 65536), halves up."""
    return int(_check_p(p) * 65536.0 + 0.5)


def scale(p: float) -> np.float32:
    """fp32(1 / (1 - p)): what kept values are multiplied by."""
    return np.float32(1.0 / (1.0 - _check_p(p)))


def stream_id(rank: int, layer: int, module_index: int) -> int:
    assert 0 <= module_index < 8 and 0 <= layer < (1 << 13) and 0 <= rank < (1 << 16)
    return (int(rank) << 16) | (int(layer) << 3) | int(module_index)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (broadcast against each other), key: two uint32 scalars or arrays -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _U32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _U32 for v in key)
    m0, m1 = np.uint64(M0), np.uint64(M1)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _U32]
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return tuple(v.astype(np.uint32) for v in c)


def keep_mask(p: float, seed: int, step: int, stream: int, rows: int, cols: int, row0: int = 0) -> np.ndarray:
    """bool [rows, cols]: True where the element (row0 + i, j) of an adapter's input is kept."""
    thr = threshold(p)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    groups = -(-int(cols) // 8)
    r = np.arange(row0, row0 + int(rows), dtype=np.uint64)[:, None]
    g = np.arange(groups, dtype=np.uint64)[None, :]
    words = philox4x32_10((r, g, np.uint64(int(stream) & 0xFFFFFFFF), np.uint64(int(step) & 0xFFFFFFFF)), (seed & 0xFFFFFFFF, seed >> 32))
    lanes = np.empty((int(rows), groups, 8), dtype=np.uint32)
    for i, w in enumerate(words):
        lanes[:, :, 2 * i] = w & np.uint32(0xFFFF)
        lanes[:, :, 2 * i + 1] = w >> np.uint32(16)
    return (lanes >= np.uint32(thr)).reshape(int(rows), groups * 8)[:, :int(cols)]
