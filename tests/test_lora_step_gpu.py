"""TrainStep(lora=LoraConfig): the reference's LoRA fine-tune (llava/train/train.py:873-889: peft adapters on every decoder linear, the projector re-enabled,
llava_arch.py:73) on the training step.  The reference is torch autograd over the oracle with W_eff = W + scaling B A built from leaf tensors A, B and the
projector (the recipe of tests/test_train_step_gpu.py); r = 8 (stored padded to 64) and B drawn non-zero so that every gradient is live."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_train_step_gpu import _rel, build_step, make_batch  # noqa: E402

pytestmark = pytest.mark.gpu

R, ALPHA = 8, 16


def _lcfg(**kw):
    from llava_mi355x.train import LoraConfig
    return LoraConfig(r=R, alpha=ALPHA, **kw)


def _draw_B(ts, seed=11):
    """The step's own A (peft's init) with B drawn N(0, 0.05^2): {name: fp32 CPU tensor}, loaded into the step."""
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.float().cpu() for k, v in ts.lora_state_dict().items()}
    for k in sd:
        if k.endswith("lora_B.weight"):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
    ts.load_lora_state_dict(sd)
    return {k: v.float().cpu() for k, v in ts.lora_state_dict().items()}            # as the step holds them (rounded to its dtype)


def lora_reference(cfg, wnp, batch, adapters, scaling, lr, max_norm, steps=1):
    from oracle import llava_oracle as O
    ids, mask, labels, pix = batch
    w = O.to_torch_weights(wnp)
    leaves = {k: v.clone().requires_grad_(True) for k, v in adapters.items()}
    leaves.update({k: v.clone().requires_grad_(True) for k, v in w.items() if "mm_projector" in k})
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    out = {}
    for _ in range(steps):
        opt.zero_grad()
        full = dict(w)
        for k in adapters:
            if k.endswith("lora_A.weight"):
                mod = k[:-len(".lora_A.weight")]
                full[mod + ".weight"] = w[mod + ".weight"] + scaling * (leaves[mod + ".lora_B.weight"] @ leaves[k])
        full.update({k: v for k, v in leaves.items() if "mm_projector" in k})
        logits, _, _, new_labels = O.llava_forward(full, cfg, ids, pix, attention_mask=mask, labels=labels)
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, cfg.vocab_size), new_labels[:, 1:].reshape(-1), ignore_index=-100)
        loss.backward()
        out.setdefault("loss", []).append(loss.item())
        if "grads" not in out:
            out["grads"] = {k: v.grad.detach().clone() for k, v in leaves.items()}
        out.setdefault("norm", []).append(float(torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm)))
        opt.step()
    with torch.no_grad():
        out["tower"] = O.vision_tower(w, cfg, pix)
    return out


def _grad(ts, k):
    kk = k.replace("model.mm_projector.", "mm_projector.")
    g = ts.g[kk]
    if kk.endswith("lora_A.weight"):
        g = g[:R]
    elif kk.endswith("lora_B.weight"):
        g = g[:, :R]
    return g


@pytest.fixture(scope="module")
def world():
    from synthetic import recipes as synth
    out = {}
    for name in ("tiny", "tiny_gqa"):
        cfg = synth.CONFIGS[name]
        out[name] = (cfg, synth.make_weights(cfg, 0), make_batch(cfg))
    return out


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_lora_step_matches_autograd_fp32(cuda, world, name):
    cfg, wnp, batch = world[name]
    lr = 1e-3
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=lr, lora=_lcfg())
    adapters = _draw_B(ts)
    ref = lora_reference(cfg, wnp, batch, adapters, ALPHA / R, lr, 1.0)
    ids, mask, labels, _ = batch
    base_before = {k: v.clone() for k, v in ts.base.items()}
    loss, _ = ts.forward_backward(ids, labels, mask, image_features=ref["tower"])
    print("loss", loss.item(), ref["loss"][0])
    assert abs(loss.item() - ref["loss"][0]) <= 1e-5 * abs(ref["loss"][0])
    worst = {k: _rel(_grad(ts, k), g) for k, g in ref["grads"].items()}
    print("worst gradient error", max(worst.values()))
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert len(worst) == 2 * 7 * cfg.num_hidden_layers + len(ts.proj_names)
    ts.optimizer_step()
    assert abs(ts.grad_norm() - ref["norm"][0]) <= 1e-4 * ref["norm"][0]
    for k, v in base_before.items():
        assert torch.equal(ts.base[k], v), k                                       # the base is bit-unchanged
    # layout: only the trainable tensors are in the flat buffers
    P = ts.part
    assert all(".lora_" in k or "mm_projector" in k for k in ts.g)
    padded = sum(-(-P.numel[k] // P.align) * P.align for k in ts.g)
    assert P.total <= padded + len(P.buckets) * P.world * P.align
    assert set(ts.p) >= set(ts.base) and "model.layers.0.self_attn.q_proj.weight" in ts.p


def test_lora_three_steps_from_peft_init(cuda, world):
    cfg, wnp, batch = world["tiny"]
    ids, mask, labels, _ = batch
    from oracle import llava_oracle as O
    with torch.no_grad():
        tower = O.vision_tower(O.to_torch_weights(wnp), cfg, batch[3])
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=2e-3, lora=_lcfg())
    assert all(float(v.abs().max()) == 0 for k, v in ts.lora_state_dict().items() if k.endswith("lora_B.weight"))       # peft: B = 0
    a0 = ts.lora_state_dict()["model.layers.0.self_attn.q_proj.lora_A.weight"]
    assert float(a0.abs().max()) <= 1 / math.sqrt(a0.shape[1]) and float(a0.abs().max()) > 0                            # kaiming_uniform_(a = sqrt(5))
    losses = [ts.step(ids, labels, mask, image_features=tower)[0].item() for _ in range(3)]
    assert losses[2] < losses[0], losses
    for k, t in ts.p.items():                                                       # the rank padding stays exactly zero
        if k.endswith("lora_A.weight"):
            assert float(t[R:].abs().max()) == 0, k
        elif k.endswith("lora_B.weight"):
            assert float(t[:, R:].abs().max()) == 0 and float(t[:, :R].abs().max()) > 0, k


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_lora_step_bf16_takes_the_rank_r_kernel(cuda, world, name):
    """tiny_gqa is the geometry where k and v are narrower than q (their dy windows of dq|dk|dv start past q at other widths) and gate / up have another width."""
    from llava_mi355x import ops
    cfg, wnp, batch = world[name]
    ts = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, lora=_lcfg())
    adapters = _draw_B(ts)
    ref = lora_reference(cfg, wnp, batch, adapters, ALPHA / R, 1e-3, 1.0)
    ids, mask, labels, _ = batch
    calls, real = {"n": 0}, ops.lora_wgrad
    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    ops.lora_wgrad = counted
    try:
        loss, _ = ts.forward_backward(ids, labels, mask, image_features=ref["tower"])
    finally:
        ops.lora_wgrad = real
    assert calls["n"] == 2 * 7 * ts.L                                               # dA and dB of every adapter went through csrc/lora.hip
    assert abs(loss.item() - ref["loss"][0]) <= 2e-2 * abs(ref["loss"][0])
    for k, g in ref["grads"].items():
        got = _grad(ts, k).float().cpu().flatten(); want = g.flatten()
        cos = float((got @ want) / (got.norm() * want.norm()).clamp_min(1e-20))
        assert cos >= 0.98, (k, cos)
    ts.optimizer_step()
    assert torch.isfinite(ts.flat_p.float()).all()


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lora_checkpointing_gives_the_same_bits(cuda, world, dtype, name):
    cfg, wnp, batch = world[name]
    ids, mask, labels, _ = batch
    from oracle import llava_oracle as O
    with torch.no_grad():
        tower = O.vision_tower(O.to_torch_weights(wnp), cfg, batch[3])
    a = build_step(cfg, wnp, dtype, cuda, lora=_lcfg())
    b = build_step(cfg, wnp, dtype, cuda, lora=_lcfg(), checkpoint=True)
    sd = _draw_B(a); b.load_lora_state_dict(sd)
    la, _ = a.forward_backward(ids, labels, mask, image_features=tower)
    lb, _ = b.forward_backward(ids, labels, mask, image_features=tower)
    assert la.item() == lb.item()
    for k in a.g:
        assert torch.equal(a.g[k], b.g[k]), k


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_lr_for_gives_the_projector_its_own_rate(cuda, world, name):
    cfg, wnp, batch = world[name]
    ids, mask, labels, _ = batch
    from oracle import llava_oracle as O
    with torch.no_grad():
        tower = O.vision_tower(O.to_torch_weights(wnp), cfg, batch[3])
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=1e-3, lora=_lcfg(), lr_for=lambda n: 0.0 if "mm_projector" in n else 1e-3)
    _draw_B(ts)
    before = ts.state_dict()
    ts.step(ids, labels, mask, image_features=tower)
    for k in ts.g:
        moved = not torch.equal(ts.p[k], before[k])
        assert moved == ("mm_projector" not in k), k
    for b, names in enumerate(ts.part.members):
        assert len({"mm_projector" in n for n in names}) == 1                      # no bucket mixes the two rates


def test_without_lora_nothing_changes(cuda, world):
    """Two steps built both ways round the new arguments' defaults: the same loss and gradient bits after forward_backward, and the same parameter bits after the
    optimiser.  The optimiser runs with clipping off: the clipping norm is an atomicAdd sum over workgroups (csrc/train.hip sumsq_kernel), whose last bits differ from
    run to run on the SAME code, before this change as after it, so parameters updated through it are not comparable bit for bit."""
    cfg, wnp, batch = world["tiny"]
    ids, mask, labels, _ = batch
    from oracle import llava_oracle as O
    with torch.no_grad():
        tower = O.vision_tower(O.to_torch_weights(wnp), cfg, batch[3])
    a = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0)
    b = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0, lora=None, lr_for=None)
    la, _ = a.forward_backward(ids, labels, mask, image_features=tower)
    lb, _ = b.forward_backward(ids, labels, mask, image_features=tower)
    assert la.item() == lb.item() and torch.equal(a.flat_g, b.flat_g)
    assert float(a.flat_g.float().abs().max()) > 0
    a.optimizer_step(); b.optimizer_step()
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.master, b.master) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert a.part.bucket_rate == [None] * len(a.part.buckets) and set(a.g) == set(a.p)
    assert a.part.buckets == b.part.buckets and a.part.offset == b.part.offset
