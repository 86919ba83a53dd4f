"""The LoRA dropout mask off the GPU: llava_mi355x/dropout.py (numpy) against Random123's known-answer vectors, against the host build of csrc/dropout.h
(lmx_dropout_keep_host), and its statistics.  The bounds are 5 sigma of the binomial the rule defines: a keep probability 1 - thr / 65536 per element, two
masks that differ in any counter word independent of each other (agreement probability (1 - q)^2 + q^2)."""
import math

import numpy as np
import pytest

SEED = 0x1234_5678_9ABC_DEF0


def _D():
    from llava_mi355x import dropout
    return dropout


def test_philox_known_answer_vectors():
    D = _D()
    hexes = lambda t: [f"{int(v):08x}" for v in t]
    assert hexes(D.philox4x32_10((0, 0, 0, 0), (0, 0))) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = 0xFFFFFFFF
    assert hexes(D.philox4x32_10((ones,) * 4, (ones, ones))) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert hexes(D.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5])
def test_host_cpp_equals_numpy(p):
    from llava_mi355x import _C
    D = _D()
    rows, cols = 192, 320
    step, stream = 3, D.stream_id(1, 5, 2)
    keep = np.full((rows, cols), 7, dtype=np.uint8)
    assert _C.lib.lmx_dropout_keep_host(p, SEED, step, stream, rows, cols, keep.ctypes.data) == 0, _C.last_error()
    assert set(np.unique(keep)) <= {0, 1}
    assert np.array_equal(keep.astype(bool), D.keep_mask(p, SEED, step, stream, rows, cols))
    # a width off the 8-column grid is the same mask cut short
    odd = np.full((rows, 13), 7, dtype=np.uint8)
    assert _C.lib.lmx_dropout_keep_host(p, SEED, step, stream, rows, 13, odd.ctypes.data) == 0
    assert np.array_equal(odd, keep[:, :13]) and np.array_equal(D.keep_mask(p, SEED, step, stream, rows, 13), keep[:, :13].astype(bool))


def test_host_cpp_refuses_bad_p():
    from llava_mi355x import _C
    keep = np.zeros((8, 8), dtype=np.uint8)
    for p in (-0.1, 1.0, 1.5):
        assert _C.lib.lmx_dropout_keep_host(p, SEED, 0, 0, 8, 8, keep.ctypes.data) != 0 and _C.last_error()


@pytest.mark.parametrize("p", [0.05, 0.1, 0.5])
def test_keep_count_is_binomial(p):
    D = _D()
    n = 256 * 4096
    q = D.threshold(p) / 65536.0
    kept = int(D.keep_mask(p, SEED, 0, 0, 256, 4096).sum())
    print("kept", kept, "expected", n * (1 - q))
    assert abs(kept - n * (1 - q)) <= 5 * math.sqrt(n * q * (1 - q))
    assert abs(q - p) <= 2.0 ** -17                          # the drop probability is p rounded to 2^-16


def test_masks_of_other_modules_layers_steps_and_ranks_are_independent():
    D = _D()
    p, rows, cols = 0.1, 256, 4096
    q = D.threshold(p) / 65536.0
    agree = (1 - q) ** 2 + q ** 2
    n = rows * cols
    base = D.keep_mask(p, SEED, 4, D.stream_id(0, 3, 1), rows, cols)
    others = {"module": D.keep_mask(p, SEED, 4, D.stream_id(0, 3, 2), rows, cols), "layer": D.keep_mask(p, SEED, 4, D.stream_id(0, 4, 1), rows, cols),
              "step": D.keep_mask(p, SEED, 5, D.stream_id(0, 3, 1), rows, cols), "rank": D.keep_mask(p, SEED, 4, D.stream_id(1, 3, 1), rows, cols),
              "seed": D.keep_mask(p, SEED + 1, 4, D.stream_id(0, 3, 1), rows, cols)}
    for what, m in others.items():
        same = int((m == base).sum())
        print(what, same / n, agree)
        assert abs(same - n * agree) <= 5 * math.sqrt(n * agree * (1 - agree)), what
    assert np.array_equal(base, D.keep_mask(p, SEED, 4, D.stream_id(0, 3, 1), rows, cols))           # a pure function
    assert np.array_equal(base[64:128], D.keep_mask(p, SEED, 4, D.stream_id(0, 3, 1), 64, cols, row0=64))
    assert D.stream_id(2, 5, 3) == 2 << 16 | 5 << 3 | 3


def test_edge_values():
    from llava_mi355x.train import LoraConfig
    D = _D()
    assert D.keep_mask(0.0, SEED, 0, 0, 64, 64).all() and D.threshold(0.0) == 0 and float(D.scale(0.0)) == 1.0
    assert D.threshold(0.05) == 3277 and D.scale(0.5) == np.float32(2.0) and D.scale(0.05).dtype == np.float32
    for bad in (-0.01, 1.0, 2.0):
        with pytest.raises(ValueError):
            D.keep_mask(bad, SEED, 0, 0, 8, 8)
        with pytest.raises(ValueError):
            LoraConfig(r=8, alpha=16, dropout=bad)
    assert LoraConfig(r=8, alpha=16, dropout=0.05).dropout == 0.05


def test_default_is_no_dropout():
    import inspect
    from llava_mi355x import train_entry
    from llava_mi355x.train import LoraConfig
    assert LoraConfig(r=8, alpha=16).dropout == 0.0
    assert inspect.signature(train_entry.train).parameters["allow_lora_dropout"].default is False
    assert inspect.signature(train_entry.save_lora_adapter).parameters["lora_dropout"].default == 0.0
