"""TrainStep(lora=LoraConfig(dropout=p)): peft's lora_dropout (y = base(x) + scaling * lora_B(lora_A(dropout(x))), one nn.Dropout per adapted linear; 0.05 in the
reference's LoRA scripts, llava/train/train.py:113, :879) on the training step.

The reference is torch autograd over the oracle.  `oracle.llava_oracle.F` is patched (monkeypatch) to a shim whose `linear` is torch's, except that for the target
weights, recognised by identity, it adds scaling * B(A(x * mask * scale)): the masks are TrainStep.lora_keep_mask (llava_mi355x/dropout.py), mapped from the step's
packed rows to [B, T] through the spliced attention mask.  Accuracy is held to the numbers tests/test_lora_step_gpu.py holds the step without dropout to."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_lora_step_gpu import ALPHA, R, _draw_B, _grad  # noqa: E402
from test_train_step_gpu import _rel, build_step, make_batch  # noqa: E402

pytestmark = pytest.mark.gpu

P_DROP = 0.1
MODS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _lcfg(**kw):
    from llava_mi355x.train import LoraConfig
    return LoraConfig(r=R, alpha=ALPHA, **kw)


class _LoraLinear:
    """torch.nn.functional with `linear` adding a dropout-masked adapter for the weights in `table` (id(weight) -> (A, B, scaling, mask [B, T, in] * scale))."""

    def __init__(self, table):
        self.table = table

    def __getattr__(self, name):
        return getattr(F, name)

    def linear(self, x, w, b=None):
        y = F.linear(x, w, b)
        hit = self.table.get(id(w))
        if hit is not None:
            A, B, scaling, m = hit
            y = y + scaling * F.linear(F.linear(x * m, A), B)
        return y


def dropout_reference(monkeypatch, ts, cfg, wnp, batch, adapters, scaling, max_norm):
    """One step of autograd + clip_grad_norm_ with the masks of ts's NEXT forward_backward call."""
    from llava_mi355x import dropout as D
    from oracle import llava_oracle as O
    ids, mask, labels, pix = batch
    w = O.to_torch_weights(wnp)
    with torch.no_grad():
        tower = O.vision_tower(w, cfg, pix)
    _, valid, _, _ = O.splice_plan(ids.numpy(), mask.numpy().astype(bool), labels.numpy(), [tower.shape[1]] * tower.shape[0], cfg.tokenizer_model_max_length,
                                   cfg.tokenizer_padding_side == "left")
    valid = torch.from_numpy(valid)
    n_rows = int(valid.sum())
    leaves = {k: v.clone().requires_grad_(True) for k, v in adapters.items()}
    leaves.update({k: v.clone().requires_grad_(True) for k, v in w.items() if "mm_projector" in k})
    full = dict(w)
    full.update({k: v for k, v in leaves.items() if "mm_projector" in k})
    table = {}
    for l in range(cfg.num_hidden_layers):
        for m in MODS:
            base = full[f"model.layers.{l}.{m}.weight"]
            keep = torch.from_numpy(ts.lora_keep_mask(l, m, n_rows, base.shape[1]))
            mm = torch.full(tuple(valid.shape) + (base.shape[1],), float(D.scale(ts.lora.dropout)))       # pad positions: any mask (nothing reads them)
            mm[valid] = keep.float() * float(D.scale(ts.lora.dropout))                                    # packed rows: sample after sample, valid positions in order
            table[id(base)] = (leaves[f"model.layers.{l}.{m}.lora_A.weight"], leaves[f"model.layers.{l}.{m}.lora_B.weight"], scaling, mm)
    monkeypatch.setattr(O, "F", _LoraLinear(table))
    logits, _, _, new_labels = O.llava_forward(full, cfg, ids, pix, attention_mask=mask, labels=labels)
    loss = F.cross_entropy(logits[:, :-1].reshape(-1, cfg.vocab_size), new_labels[:, 1:].reshape(-1), ignore_index=-100)
    loss.backward()
    monkeypatch.undo()
    grads = {k: v.grad.detach().clone() for k, v in leaves.items()}
    norm = float(torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm))
    return {"loss": loss.item(), "grads": grads, "norm": norm, "tower": tower}


@pytest.fixture(scope="module")
def world():
    from oracle import llava_oracle as O
    from synthetic import recipes as synth
    out = {}
    for name in ("tiny", "tiny_gqa"):
        cfg = synth.CONFIGS[name]
        wnp = synth.make_weights(cfg, 0)
        batch = make_batch(cfg)
        with torch.no_grad():
            tower = O.vision_tower(O.to_torch_weights(wnp), cfg, batch[3])
        out[name] = (cfg, wnp, batch, tower)
    return out


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_dropout_step_matches_autograd_fp32(cuda, world, monkeypatch, name):
    cfg, wnp, batch, _ = world[name]
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=1e-3, lora=_lcfg(dropout=P_DROP), dropout_seed=1234)
    adapters = _draw_B(ts)
    ts.dropout_step = 3                                                             # not the first call: the step word of the counter is live
    ref = dropout_reference(monkeypatch, ts, cfg, wnp, batch, adapters, ALPHA / R, 1.0)
    ids, mask, labels, _ = batch
    loss, _ = ts.forward_backward(ids, labels, mask, image_features=ref["tower"])
    assert ts.dropout_step == 4
    print("loss", loss.item(), ref["loss"])
    assert abs(loss.item() - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    worst = {k: _rel(_grad(ts, k), g) for k, g in ref["grads"].items()}
    print("worst gradient error", max(worst.values()))
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert len(worst) == 2 * 7 * cfg.num_hidden_layers + len(ts.proj_names)
    ts.optimizer_step()
    assert abs(ts.grad_norm() - ref["norm"]) <= 1e-4 * ref["norm"]
    # and the masks matter: the step without them is outside the same bound
    plain = build_step(cfg, wnp, torch.float32, cuda, lr=1e-3, lora=_lcfg())
    plain.load_lora_state_dict(adapters)
    l0, _ = plain.forward_backward(ids, labels, mask, image_features=ref["tower"])
    assert abs(l0.item() - ref["loss"]) > 1e-5 * abs(ref["loss"])


@pytest.mark.parametrize("name", ["tiny", "tiny_gqa"])
def test_bf16_step_takes_the_fused_kernels_and_recompute_regenerates_the_masks(cuda, world, name):
    from llava_mi355x import ops
    cfg, wnp, batch, tower = world[name]
    ids, mask, labels, _ = batch
    L = cfg.num_hidden_layers
    a = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(dropout=P_DROP), checkpoint=True, keep_layers=0)
    b = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(dropout=P_DROP), checkpoint=True, keep_layers=L)
    sd = _draw_B(a); b.load_lora_state_dict(sd)
    seen = {"down_ok": [], "wgrad_ok": [], "down": 0, "wgrad": 0, "materialised": []}
    real = {n: getattr(ops, n) for n in ("lora_down_dropout_ok", "lora_wgrad_ok", "lora_down_dropout", "lora_wgrad_dropout", "dropout")}

    def wrap(name, key, count):
        def f(*args, **kw):
            out = real[name](*args, **kw)
            if count:
                seen[key] += 1
            else:
                seen[key].append(out if key != "materialised" else tuple(args[0].shape))
            return out
        return f
    ops.lora_down_dropout_ok, ops.lora_wgrad_ok = wrap("lora_down_dropout_ok", "down_ok", False), wrap("lora_wgrad_ok", "wgrad_ok", False)
    ops.lora_down_dropout, ops.lora_wgrad_dropout = wrap("lora_down_dropout", "down", True), wrap("lora_wgrad_dropout", "wgrad", True)
    ops.dropout = wrap("dropout", "materialised", False)
    try:
        la, _ = a.forward_backward(ids, labels, mask, image_features=tower)
        counts = (seen["down"], seen["wgrad"])
        lb, _ = b.forward_backward(ids, labels, mask, image_features=tower)
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
    assert seen["down_ok"] and all(seen["down_ok"]) and seen["wgrad_ok"] and all(seen["wgrad_ok"])    # every call was accepted by its fused kernel
    assert counts == (2 * 4 * L, 7 * L)                       # a: q|k|v, o, gate|up, down per layer in the forward and again in the recompute; dA of every adapter
    assert (seen["down"], seen["wgrad"]) == (3 * 4 * L, 2 * 7 * L) and a.last_kept_layers == 0 and b.last_kept_layers == L
    # ops.dropout only ever ran on t = du A of a chain's first adapter ([rows, in] of down, gate, o and q: four per layer), never to materialise a masked x for a GEMM
    assert len(seen["materialised"]) == 2 * 4 * L
    assert la.item() == lb.item()
    for k in a.g:
        assert torch.equal(a.g[k], b.g[k]), k                                        # recompute regenerated the same masks
    assert float(a.flat_g.float().abs().max()) > 0 and torch.isfinite(a.flat_g.float()).all()


def test_counter_and_seed(cuda, world):
    cfg, wnp, batch, tower = world["tiny"]
    ids, mask, labels, _ = batch
    ts = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(dropout=P_DROP), lora_seed=3)
    assert ts.dropout_seed == 3 and ts.dropout_step == 0                             # the seed defaults to lora_seed
    sd = _draw_B(ts)
    l0, _ = ts.forward_backward(ids, labels, mask, image_features=tower)
    g0 = ts.flat_g.clone()
    assert ts.dropout_step == 1
    l1, _ = ts.forward_backward(ids, labels, mask, image_features=tower)           # no optimiser step in between: two micro-batches of one accumulation
    assert ts.dropout_step == 2 and l1.item() != l0.item() and not torch.equal(ts.flat_g, g0)
    ts.dropout_step = 0
    l2, _ = ts.forward_backward(ids, labels, mask, image_features=tower)
    assert l2.item() == l0.item() and torch.equal(ts.flat_g, g0)                     # the same seed and step: the same bits
    assert np.array_equal(ts.lora_keep_mask(0, "q_proj", 8, 64, step=0), ts.lora_keep_mask(0, "self_attn.q_proj", 8, 64, step=0))
    assert not np.array_equal(ts.lora_keep_mask(0, "q_proj", 8, 64, step=0), ts.lora_keep_mask(0, "k_proj", 8, 64, step=0))
    other = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(dropout=P_DROP), lora_seed=3, dropout_seed=4)
    other.load_lora_state_dict(sd)
    l3, _ = other.forward_backward(ids, labels, mask, image_features=tower)
    assert l3.item() != l0.item()
    l4, _ = ts.forward_backward(ids, labels, mask, image_features=tower, backward=False, dropout=True)
    assert ts.dropout_step == 2 and l4.item() == l1.item()                          # a forward-only look at the training loss: step 1's masks, on request
    # a plain forward-only call is an evaluation (peft: nn.Dropout is the identity in eval mode): the adapters unmasked, the counter where it was
    plain = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(), lora_seed=3)
    plain.load_lora_state_dict(sd)
    want, _ = plain.forward_backward(ids, labels, mask, image_features=tower, backward=False)
    l5, _ = ts.forward_backward(ids, labels, mask, image_features=tower, backward=False)
    assert ts.dropout_step == 2 and l5.item() == want.item() and l5.item() != l1.item()
    l6, _ = ts.forward_backward(ids, labels, mask, image_features=tower)            # the training masks did not shift
    ts.dropout_step = 2
    l7, _ = ts.forward_backward(ids, labels, mask, image_features=tower)
    assert l6.item() == l7.item() and ts.dropout_step == 3


def test_a_target_subset_with_a_gap_takes_the_kernel_one_adapter_at_a_time(cuda, world):
    """target_modules = (q_proj, v_proj): the group's streams (module indices 0 and 2) are not consecutive, so the down kernel runs once per adapter with G = 1.
    Each window of u against float64 of ops.dropout's output under that adapter's own stream, with the bound of tests/test_lora_dropout_kernels_gpu.py."""
    from llava_mi355x import ops
    cfg, wnp, batch, tower = world["tiny"]
    ts = build_step(cfg, wnp, torch.bfloat16, cuda, lora=_lcfg(dropout=P_DROP, target_modules=("q_proj", "v_proj")), dropout_seed=21)
    assert ts.lora_groups[(0, "self_attn.q_proj")] == ("self_attn.q_proj", "self_attn.v_proj")
    g = torch.Generator(device="cpu").manual_seed(4)
    rows, K = 128, ts.H
    h = torch.randn((rows, K), generator=g).to(torch.bfloat16).to(cuda)
    calls, real = [], ops.lora_down_dropout
    def counted(x, A, G, p, seed, step, stream0, out=None):
        calls.append((G, stream0))
        return real(x, A, G, p, seed, step, stream0, out=out)
    ops.lora_down_dropout = counted
    try:
        us = ts._lora_down(1, "self_attn.q_proj", h)
    finally:
        ops.lora_down_dropout = real
    assert calls == [(1, 1 << 3 | 0), (1, 1 << 3 | 2)]
    for m, idx in (("self_attn.q_proj", 0), ("self_attn.v_proj", 2)):
        A = ts.p[f"model.layers.1.{m}.lora_A.weight"].double()
        xd = ops.dropout(h, P_DROP, 21, 0, 1 << 3 | idx).double()
        ref = xd @ A.t()
        tol = 2.0 ** -8 * ref.abs() + 2 * K * 2.0 ** -24 * (xd.abs() @ A.abs().t())
        assert ((us[m].double() - ref).abs() <= tol).all(), m
        assert float(us[m][:, :R].abs().max()) > 0 and float(us[m][:, R:].abs().max()) == 0       # the rank padding stays zero
    # and the whole step runs on that tier: loss and gradients finite, k_proj has no adapter
    ids, mask, labels, _ = batch
    loss, _ = ts.forward_backward(ids, labels, mask, image_features=tower)
    assert torch.isfinite(loss) and torch.isfinite(ts.flat_g.float()).all() and not any("k_proj.lora" in k for k in ts.g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dropout_zero_is_the_step_without_the_field(cuda, world, dtype):
    from llava_mi355x import ops
    from llava_mi355x.train import LoraConfig
    cfg, wnp, batch, tower = world["tiny"]
    ids, mask, labels, _ = batch
    a = build_step(cfg, wnp, dtype, cuda, lora=LoraConfig(r=R, alpha=ALPHA))
    b = build_step(cfg, wnp, dtype, cuda, lora=LoraConfig(r=R, alpha=ALPHA, dropout=0.0), dropout_seed=99)
    sd = _draw_B(a); b.load_lora_state_dict(sd)
    names = ("dropout", "dropout_add", "lora_down_dropout", "lora_wgrad_dropout")
    real = {n: getattr(ops, n) for n in names}

    def refuse(*a, **kw):
        raise AssertionError("a dropout kernel ran at p = 0")
    for n in names:
        setattr(ops, n, refuse)
    try:
        la, _ = a.forward_backward(ids, labels, mask, image_features=tower)
        lb, _ = b.forward_backward(ids, labels, mask, image_features=tower)
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
    assert la.item() == lb.item() and torch.equal(a.flat_g, b.flat_g)
    assert b.lora_keep_mask(0, "q_proj", 4, 16).all()


def test_entry_point_trains_with_dropout_and_records_it(cuda, tmp_path):
    from ckpt_util import write_clip, write_llava
    from test_lora_roundtrip_gpu import _margs
    from test_train_entry_gpu import _args, _world
    from llava_mi355x import conversation as C, train_data as D, train_entry as E
    from llava_mi355x.builder import load_pretrained_model
    from synthetic import recipes as synth
    cfg, lc, weights, tok, tower, data_args, model = _world(tmp_path)
    wnp = synth.make_weights(cfg, 0)
    clip_dir = str(tmp_path / "clip-tiny")
    write_clip(clip_dir, cfg, wnp, "4.31")
    base = str(tmp_path / "vicuna-tiny")
    write_llava(base, cfg, wnp, clip_dir, with_projector=False)
    targs = _args(D, tmp_path, lora_enable=True, lora_r=8, lora_alpha=16, lora_dropout=0.05, max_steps=2, learning_rate=2e-3, mm_projector_lr=2e-4)
    targs.output_dir = str(tmp_path / "llava-tiny-lora")
    keep = C.default_conversation
    try:
        with pytest.raises(NotImplementedError, match="LoRA dropout is not implemented"):      # the default still refuses, word for word
            E.train(_margs(D, cfg, clip_dir), data_args, targs, config=lc, weights=weights, tokenizer=tok, vision_tower=tower)
        out = E.train(_margs(D, cfg, clip_dir), data_args, targs, config=lc, weights=weights, tokenizer=tok, vision_tower=tower, allow_lora_dropout=True)
    finally:
        C.default_conversation = keep
    ts = out["train_step"]
    assert out["steps"] == 2 and all(np.isfinite(out["losses"])) and ts.lora.dropout == 0.05 and ts.dropout_step == 2 and ts.dropout_seed == int(targs.seed)
    ac = json.load(open(os.path.join(targs.output_dir, "adapter_config.json")))
    assert ac["lora_dropout"] == 0.05 and ac["r"] == 8
    assert any(float(v.abs().max()) > 0 for k, v in ts.lora_state_dict().items() if k.endswith("lora_B.weight"))
    tokenizer, loaded, _, _ = load_pretrained_model(targs.output_dir, base, "llava-tiny-lora", torch_dtype=torch.float32)
    ids_np = synth.make_prompt(cfg, 12, image_positions=(5,))
    ids_np[ids_np >= 0] %= len(tokenizer)
    logits = loaded.forward(input_ids=torch.from_numpy(ids_np)[None].to(cuda), images=torch.from_numpy(synth.make_pixels(cfg, 1)).to(cuda), use_cache=False).logits
    assert torch.isfinite(logits).all()
