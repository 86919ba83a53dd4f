"""Host-side conditions of tests/test_linears_fp64_gpu.py, checked without a device: the case table reaches every gemv2_body instantiation that launch_gemv2 can
select, and for the seeds in use the flippable set of the RMSNorm prologue (linear_ref.norm_chain) stays under its cap in every case — the cap is a term of the bound
that could hide a failure, so the condition is part of the test."""
import pytest
import torch

import linear_ref as L
import test_linears_fp64_gpu as G


def test_gemv2_case_table_reaches_every_instantiation():
    got = {p.values[0]["cfg"] for p in G.GEMV2_CASES}
    assert G.REACHABLE <= got and None in got, sorted(G.REACHABLE - got)
    for p in G.GEMV2_CASES:
        c = p.values[0]
        assert c["K"] % 8 == 0 and (c["act"] != G.SILU or c["N"] % 64 == 0)


def test_flippable_set_is_under_the_cap_for_every_case():
    worst = {}
    for label, dt, x in G.host_norm_inputs():
        f = L.flip_fraction(x, dt)
        assert f <= L.FLIP_MAX_FRACTION, f"{label} {dt}: {f:.4f} of K on a rounding boundary; pick another SALT"
        worst[dt] = max(worst.get(dt, 0.0), f)
    print("worst flippable fraction", worst)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_flippable_mask_covers_an_fp32_prologue(dt):
    """norm_chain's mask against a host restatement of the kernels' prologue (fp32 sum of squares, fp32 rsqrt, fp32 product rounded to T): wherever that lands on
    another value of T than the float64 chain, the element must be marked.  400 rows per dtype, among them rows whose mask is not empty (flips cluster by row: they
    depend on inv, a bf16 row has about K / 128 of them or none), so the mask is exercised for bf16 although the seeds in use leave every bf16 case without one."""
    g = torch.Generator().manual_seed(17)
    K = 1024
    x = torch.randn(400, K, generator=g).to(L.DT[dt])
    p, mask = L.norm_chain(x, dt, 1e-5)
    xf = x.float()
    inv32 = torch.rsqrt(xf.pow(2).sum(-1, keepdim=True) / K + 1e-5)
    a32 = (xf * inv32).to(L.DT[dt]).double()
    moved = a32 != L.rnd(p, dt)
    assert int(mask.sum()) > 0 and int((mask.sum(-1) > 0).sum()) >= 2, "no row of this sample has a flippable element: the check below would be empty"
    assert not bool((moved & ~mask).any()), f"{int((moved & ~mask).sum())} elements moved by the fp32 prologue are outside the flippable set"
    print(dt, "rows with flips", int((mask.sum(-1) > 0).sum()), "marked", int(mask.sum()), "moved", int(moved.sum()))
