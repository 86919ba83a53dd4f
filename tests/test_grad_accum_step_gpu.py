"""Gradient accumulation on the training step (TrainStep.forward_backward(micro=(i, n)), accumulate_step, train_entry.train with gradient_accumulation_steps > 1):
what the reference's scripts ask of HF Trainer with --gradient_accumulation_steps (each micro-batch back-propagates its mean loss / n, torch adds into .grad, one
clip + AdamW step on the sum).  `tiny` synthetic config throughout; the step recipe, helpers and tolerances are those of tests/test_train_step_gpu.py and
tests/test_lora_step_gpu.py.

The two micro-batches are make_batch(cfg, 0) and make_batch(cfg, 1).  make_batch masks the same positions whatever its seed, so the two would count the same
number of labels and a mean of the micro-batch means would equal a mean over all their positions; `_batches` therefore masks six more positions of the second one's
first sample, which makes the counts differ (asserted below) and a joint mean a different number from the (loss_0 + loss_1) / 2 that HF Trainer optimises."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_train_step_gpu import _free_port, _rel, build_step, make_batch, trainable  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _batches(cfg):
    b0, b1 = make_batch(cfg, 0), make_batch(cfg, 1)
    ids, mask, labels, pix = b1
    labels = labels.clone(); labels[0, :15] = -100
    return [b0, (ids, mask, labels, pix)]


@pytest.fixture(scope="module")
def world():
    """cfg, weights, the two micro-batches, the frozen tower's features of each and the forward_backward argument tuples: built once."""
    from oracle import llava_oracle as O
    from synthetic import recipes as synth
    cfg = synth.CONFIGS["tiny"]
    wnp = synth.make_weights(cfg, 0)
    batches = _batches(cfg)
    w = O.to_torch_weights(wnp)
    with torch.no_grad():
        towers = [O.vision_tower(w, cfg, b[3]) for b in batches]
    micro = [(b[0], b[2], b[1], t) for b, t in zip(batches, towers)]              # forward_backward's order: ids, labels, mask, features
    return cfg, wnp, batches, micro


def _accum_reference(cfg, w, leaves, build_full, batches, lr, max_norm):
    """torch autograd over the oracle: (loss_0 + loss_1) / 2 -> backward -> clip_grad_norm_ -> one AdamW step (what HF Trainer does with accumulation)."""
    from oracle import llava_oracle as O
    opt = torch.optim.AdamW(list(leaves.values()), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    opt.zero_grad()
    losses, counts = [], []
    for ids, mask, labels, pix in batches:
        logits, _, _, new_labels = O.llava_forward(build_full(), cfg, ids, pix, attention_mask=mask, labels=labels)
        losses.append(F.cross_entropy(logits[:, :-1].reshape(-1, cfg.vocab_size), new_labels[:, 1:].reshape(-1), ignore_index=-100))
        counts.append(int((new_labels[:, 1:] != -100).sum()))
    (sum(losses) / len(losses)).backward()
    out = {"losses": [l.item() for l in losses], "counts": counts, "grads": {k: v.grad.detach().clone() for k, v in leaves.items()}}
    out["norm"] = float(torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm))
    opt.step()
    out["params"] = {k: v.detach().clone() for k, v in leaves.items()}
    return out


def test_accumulate_step_matches_autograd_and_adamw_fp32(cuda, world):
    """Loss, every gradient, the clipping norm and every parameter after the step under the tolerances of test_one_step_matches_autograd_and_adamw_fp32."""
    from oracle import llava_oracle as O
    cfg, wnp, batches, micro = world
    lr, wd, max_norm = 1e-3, 0.0, 1.0
    w = O.to_torch_weights(wnp)
    params = {k: v.clone().requires_grad_(True) for k, v in w.items() if trainable(k)}
    def full():
        f = dict(w); f.update(params)
        return f
    ref = _accum_reference(cfg, w, params, full, batches, lr, max_norm)
    assert ref["counts"][0] != ref["counts"][1]                                  # a mean of means is not the joint mean here
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
    before = ts.state_dict()
    grads = {}
    real = ts.optimizer_step
    def spy():
        grads.update({k: v.detach().clone() for k, v in ts.g.items()})
        real()
    ts.optimizer_step = spy
    loss, count = ts.accumulate_step(micro)
    want_loss = sum(ref["losses"]) / 2
    print("loss", loss.item(), want_loss, "counts", ref["counts"])
    assert int(count.item()) == sum(ref["counts"])
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    worst = {k: _rel(grads[k.replace("model.mm_projector.", "mm_projector.")], g) for k, g in ref["grads"].items()}
    print("worst gradient error", max(worst.values()))
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert abs(ts.grad_norm() - ref["norm"]) <= 1e-4 * ref["norm"]
    w0 = {k: torch.from_numpy(v) for k, v in wnp.items()}
    for k, p_ref in ref["params"].items():
        kk = k.replace("model.mm_projector.", "mm_projector.")
        d_ref = p_ref - w0[k]
        d_got = ts.p[kk].detach().cpu() - before[kk].cpu()
        g = ref["grads"][k]
        solid = g.abs() > 1e-3 * g.abs().max()
        if solid.any():
            assert (d_got[solid] - d_ref[solid]).abs().max().item() <= 1e-2 * lr, k
        assert (d_got - d_ref).abs().max().item() <= 2.001 * lr, k
        assert float(d_got[g == 0].abs().max() if (g == 0).any() else 0.0) == 0.0, k


def test_accumulate_step_with_lora_matches_autograd_fp32(cuda, world):
    """The same with rank-8 adapters: helpers and tolerances of tests/test_lora_step_gpu.py::test_lora_step_matches_autograd_fp32."""
    from oracle import llava_oracle as O
    from test_lora_step_gpu import ALPHA, R, _draw_B, _grad, _lcfg
    cfg, wnp, batches, micro = world
    lr = 1e-3
    ts = build_step(cfg, wnp, torch.float32, cuda, lr=lr, lora=_lcfg())
    adapters = _draw_B(ts)
    scaling = ALPHA / R
    w = O.to_torch_weights(wnp)
    leaves = {k: v.clone().requires_grad_(True) for k, v in adapters.items()}
    leaves.update({k: v.clone().requires_grad_(True) for k, v in w.items() if "mm_projector" in k})
    def full():
        f = dict(w)
        for k in adapters:
            if k.endswith("lora_A.weight"):
                mod = k[:-len(".lora_A.weight")]
                f[mod + ".weight"] = w[mod + ".weight"] + scaling * (leaves[mod + ".lora_B.weight"] @ leaves[k])
        f.update({k: v for k, v in leaves.items() if "mm_projector" in k})
        return f
    ref = _accum_reference(cfg, w, leaves, full, batches, lr, 1.0)
    grads = {}
    real = ts.optimizer_step
    def spy():
        grads.update({k: _grad(ts, k).detach().clone() for k in ref["grads"]})
        real()
    ts.optimizer_step = spy
    loss, count = ts.accumulate_step(micro)
    want_loss = sum(ref["losses"]) / 2
    assert int(count.item()) == sum(ref["counts"])
    assert abs(loss.item() - want_loss) <= 1e-5 * abs(want_loss)
    worst = {k: _rel(grads[k], g) for k, g in ref["grads"].items()}
    print("worst gradient error", max(worst.values()))
    bad = {k: v for k, v in worst.items() if v > 1e-3}
    assert not bad, bad
    assert len(worst) == 2 * 7 * cfg.num_hidden_layers + len(ts.proj_names)
    assert abs(ts.grad_norm() - ref["norm"]) <= 1e-4 * ref["norm"]


def test_bf16_accumulation_rounds_once_per_micro_batch_on_the_direct_kernels(cuda, world):
    """g1, g2: the gradients of each micro-batch alone (both as micro-batch 0 of 2, i.e. scaled by 1 / 2); acc: after (0, 2) on the first and (1, 2) on the second.
    |acc - (g1 + g2)| <= u (|g1 + g2| + |g2|), u = 2^-8: half an ulp for acc's rounding, half an ulp for g2's own rounding, and the same again as margin for the
    order of the fp32 atomics in the embedding table.  Every decoder linear and lm_head must take the accumulating form of the direct kernel in micro-batch 1."""
    from llava_mi355x import ops
    cfg, wnp, batches, micro = world
    a = build_step(cfg, wnp, torch.bfloat16, cuda)
    b = build_step(cfg, wnp, torch.bfloat16, cuda)
    c = build_step(cfg, wnp, torch.bfloat16, cuda)
    a.forward_backward(*micro[0], micro=(0, 2))
    g1 = {k: v.double().clone() for k, v in a.g.items()}
    b.forward_backward(*micro[1], micro=(0, 2))
    g2 = {k: v.double().clone() for k, v in b.g.items()}
    calls, real = [], ops.gemm_wgrad
    def counted(*args, **kw):
        calls.append(bool(kw.get("accumulate", False)))
        return real(*args, **kw)
    ops.gemm_wgrad = counted
    try:
        c.forward_backward(*micro[0], micro=(0, 2))
        n0, acc0 = len(calls), sum(calls)
        c.forward_backward(*micro[1], micro=(1, 2))
    finally:
        ops.gemm_wgrad = real
    assert n0 >= 5 * c.L + 1 and acc0 == 0                               # micro-batch 0 overwrites
    assert sum(calls) >= 5 * c.L + 1 and all(calls[n0:])                 # micro-batch 1: q|k|v, o, gate, up, down per layer + lm_head, all accumulating
    u = 2.0 ** -8
    for k in c.g:
        s = g1[k] + g2[k]
        over = (c.g[k].double() - s).abs() - u * (s.abs() + g2[k].abs())
        assert over.max().item() <= 0, (k, over.max().item())
        assert float(g2[k].abs().max()) > 0, k                           # the second micro-batch really adds something everywhere
    c.optimizer_step()
    assert torch.isfinite(c.flat_p.float()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_checkpointing_gives_the_same_accumulated_bits(cuda, world, dtype):
    cfg, wnp, batches, micro = world
    a = build_step(cfg, wnp, dtype, cuda)
    b = build_step(cfg, wnp, dtype, cuda, checkpoint=True)
    for i in range(2):
        la, _ = a.forward_backward(*micro[i], micro=(i, 2))
        lb, _ = b.forward_backward(*micro[i], micro=(i, 2))
        assert la.item() == lb.item()
    for k in a.g:
        assert torch.equal(a.g[k], b.g[k]), k


def test_default_path_is_unchanged_and_a_plain_call_still_overwrites(cuda, world):
    """micro=None against the explicit (0, 1) and against a step that never heard of micro-batches: the same loss, gradient and (clipping off: its norm is an
    atomicAdd sum) parameter bits; a second plain call overwrites the gradients of the first."""
    cfg, wnp, batches, micro = world
    a = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0)
    b = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0)
    la, _ = a.forward_backward(*micro[0])
    lb, _ = b.forward_backward(*micro[0], micro=(0, 1))
    assert la.item() == lb.item() and torch.equal(a.flat_g, b.flat_g) and float(a.flat_g.float().abs().max()) > 0
    a.optimizer_step(); b.optimizer_step()
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.master, b.master)
    c = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0)
    d = build_step(cfg, wnp, torch.bfloat16, cuda, lr=1e-3, max_grad_norm=0.0)
    c.forward_backward(*micro[0])
    c.forward_backward(*micro[1])                                        # plain: overwrites what the first call left
    d.forward_backward(*micro[1])
    assert torch.equal(c.flat_g, d.flat_g)


def test_optimizer_step_refuses_an_unfinished_accumulation(cuda, world):
    cfg, wnp, batches, micro = world
    ts = build_step(cfg, wnp, torch.bfloat16, cuda)
    with pytest.raises(RuntimeError, match="micro-batch"):
        ts.forward_backward(*micro[1], micro=(1, 2))                     # nothing to accumulate into
    ts.forward_backward(*micro[0], micro=(0, 2))
    before = ts.flat_p.clone()
    with pytest.raises(RuntimeError, match="accumulation"):
        ts.optimizer_step()
    assert torch.equal(ts.flat_p, before) and ts.step_count == 0
    ts.forward_backward(*micro[1], micro=(1, 2))
    ts.optimizer_step()
    assert ts.step_count == 1 and not torch.equal(ts.flat_p, before)
    with pytest.raises(ValueError):
        ts.forward_backward(*micro[0], micro=(2, 2))


def test_zero2_two_ranks_accumulate_locally_and_reduce_once(cuda, tmp_path):
    """The harness of test_zero2_two_ranks_match_single_rank (gloo, two processes on this GPU).  Both ranks run the same two micro-batches: after the update they hold
    the single-rank accumulated step's parameters under that test's criterion, and every bucket was reduce-scattered once, in the last micro-batch."""
    port = _free_port()
    procs = []
    for r in range(2):
        out = str(tmp_path / f"ga{r}.pt")
        procs.append((subprocess.Popen([sys.executable, os.path.join(HERE, "grad_accum_worker.py"), str(r), "2", str(port), out], stdout=subprocess.PIPE,
                                       stderr=subprocess.STDOUT), out))
    logs = []
    for p, _ in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill(); o, _ = p.communicate()
        logs.append(o.decode(errors="replace")[-2500:])
    res = []
    for (_, out), lg in zip(procs, logs):
        assert os.path.exists(out), lg
        res.append(torch.load(out))
    for r in res:
        assert r["ok"], r.get("trace")
    nb = res[0]["n_buckets"]
    assert nb > 3
    for r in res:
        assert r["scatters_after_micro0"] == []                                         # micro-batch 0 accumulates locally
        assert sorted(r["scatters_after_micro1"]) == list(range(nb))                    # every bucket once, under micro-batch 1's backward
        assert r["scatters_after_step"] == r["scatters_after_micro1"]                   # the optimiser reduces nothing again
    assert torch.equal(res[0]["params"], res[1]["params"])
    single = res[0]["single_params"]
    diff = (res[0]["params"] - single).abs()
    assert diff.max().item() <= 2.001e-3 and (diff > 1e-6).float().mean().item() < 1e-2
    assert abs(res[0]["norm"] - res[0]["single_norm"]) <= 1e-5 * res[0]["single_norm"]


@pytest.mark.parametrize("GA", [2, 1])
def test_train_entry_walks_micro_batch_indices(cuda, tmp_path, GA):
    """train() with gradient_accumulation_steps = GA, batch 1, two optimiser steps, on the fixture of tests/test_train_entry_gpu.py (the projector stage, clipping
    off: nothing in the run sums with atomics, so the bits are comparable) against a TrainStep driven by hand over micro_batch_indices — for GA = 1 over today's
    slices order[(b * world + rank) * B:][:B] and TrainStep.step.  The records hold the mean of the micro-batch losses and the sum of their label counts."""
    from llava_mi355x import conversation as C, train_data as D, train_entry as E
    from llava_mi355x.train import TrainStep
    from test_train_entry_gpu import _args, _world
    cfg, lc, weights, tok, tower, data_args, model = _world(tmp_path)
    before = {k: v.clone() for k, v in weights.items()}
    margs = D.ModelArguments(model_name_or_path="synthetic", version="plain", vision_tower="synthetic-clip", mm_vision_select_layer=cfg.mm_vision_select_layer,
                             mm_projector_type=cfg.mm_projector_type, tune_mm_mlp_adapter=True, mm_use_im_start_end=False, mm_use_im_patch_token=False)
    targs = _args(D, tmp_path, per_device_train_batch_size=1, gradient_accumulation_steps=GA, max_steps=2, max_grad_norm=0.0)
    records = []
    keep = C.default_conversation
    try:
        out = E.train(margs, data_args, targs, config=lc, weights=weights, tokenizer=tok, vision_tower=tower, log=records.append)
        assert out["steps"] == 2 and len(out["losses"]) == 2
        state = json.load(open(tmp_path / "out" / "trainer_state.json"))
        assert state["global_step"] == 2 and [r["step"] for r in state["log_history"]] == [1, 2]
        # ---- the same run by hand (train() left its settings in lc, data_args and the tokenizer) -----------------------------------------------------------
        module = D.make_supervised_data_module(tokenizer=tok, data_args=data_args)
        dataset, collate = module["train_dataset"], module["data_collator"]
        ts = TrainStep(lc, {k: v for k, v in before.items() if "vision_tower" not in k and not k.startswith("vision.")}, dtype=torch.float32, device="cuda",
                       lr=targs.learning_rate, betas=(targs.adam_beta1, targs.adam_beta2), eps=targs.adam_epsilon, weight_decay=targs.weight_decay,
                       max_grad_norm=targs.max_grad_norm, max_positions=max(2048, int(tok.model_max_length) + 1024), lora_seed=targs.seed, dropout_seed=targs.seed)
        frozen = set(out["frozen"])
        ts.set_trainable(lambda name: (("model." + name) if name.startswith("mm_projector.") else name) not in frozen)
        order = torch.randperm(len(dataset), generator=torch.Generator().manual_seed(int(targs.seed))).tolist()
        hand = []
        for update in range(2):
            ts.lr = E.lr_at(update, 2, targs.learning_rate, targs.warmup_ratio, targs.lr_scheduler_type)
            micro = []
            for i in range(GA):
                idx = E.micro_batch_indices(order, update, i, 0, 1, 1, GA)
                if GA == 1:
                    assert idx == order[update:update + 1]
                batch = collate([dataset[j] for j in idx])
                feats = tower(batch["images"].to(device="cuda", dtype=torch.float32))
                micro.append((batch["input_ids"], batch["labels"], batch["attention_mask"], feats))
            if GA == 1:
                loss, count = ts.step(*micro[0])
            else:
                loss, count = ts.accumulate_step(micro)
            hand.append((float(loss.item()), int(count)))
    finally:
        C.default_conversation = keep
    want = ts.state_dict()
    assert set(want) == set(out["state"])
    for k, v in want.items():
        assert torch.equal(out["state"][k], v), k                        # bit-equal, moved tensors and frozen ones alike
    moved = [k for k in want if not torch.equal(want[k].cpu().float(), before[("model." + k) if k.startswith("mm_projector.") else k].float())]
    assert moved and all("mm_projector" in k for k in moved)
    assert [(r["loss"], r["label_positions"]) for r in records] == hand


def test_train_entry_runs_the_llava_plus_recipe_arguments(cuda, tmp_path):
    """The arguments of the reference's scripts/llava_plus/training_llava_plus_v1.3_7b.sh that the entry reads (--version v1, --gradient_accumulation_steps 2, 3 epochs,
    2e-5 cosine with 3 % warm-up, weight decay 0, gradient checkpointing, logging every step) on the fixture of tests/test_train_entry_gpu.py, whose eight samples and
    fp32 tower ask for batch 2 and the fp32 engine in place of the script's 16 and bf16: (8 // 2) // 2 = 2 optimiser steps per epoch, 6 in all.  The script's own
    batch of 16 does not fill one optimiser step of this dataset and is refused by name."""
    import math
    from llava_mi355x import conversation as C, train_data as D, train_entry as E
    from test_train_entry_gpu import _args, _world
    cfg, lc, weights, tok, tower, data_args, model = _world(tmp_path)
    margs = D.ModelArguments(model_name_or_path="synthetic", version="v1", vision_tower="synthetic-clip", mm_vision_select_layer=cfg.mm_vision_select_layer,
                             mm_projector_type=cfg.mm_projector_type, mm_use_im_start_end=False, mm_use_im_patch_token=False)
    recipe = dict(gradient_accumulation_steps=2, num_train_epochs=3, learning_rate=2e-5, weight_decay=0.0, warmup_ratio=0.03, lr_scheduler_type="cosine",
                  logging_steps=1, gradient_checkpointing=True)
    records = []
    keep = C.default_conversation
    try:
        with pytest.raises(ValueError, match="gradient_accumulation_steps"):
            E.train(margs, data_args, _args(D, tmp_path, per_device_train_batch_size=16, **recipe), config=lc, weights={k: v.clone() for k, v in weights.items()},
                    tokenizer=tok, vision_tower=tower)
        out = E.train(margs, data_args, _args(D, tmp_path, per_device_train_batch_size=2, **recipe), config=lc, weights=weights, tokenizer=tok, vision_tower=tower,
                      log=records.append)
    finally:
        C.default_conversation = keep
    assert out["steps"] == 6 and len(records) == 6 and [r["step"] for r in records] == [1, 2, 3, 4, 5, 6]
    assert all(math.isfinite(r["loss"]) and r["label_positions"] > 0 for r in records)
    assert [r["learning_rate"] for r in records] == [E.lr_at(s, 6, 2e-5, 0.03, "cosine") for s in range(6)]       # the schedule counts optimiser steps
    assert json.load(open(tmp_path / "out" / "trainer_state.json"))["global_step"] == 6
    assert out["train_step"].checkpoint and out["train_step"].step_count == 6
