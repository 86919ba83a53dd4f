"""LoRA measurements on one GPU (results: profiles/EXPERIMENTS.md, "LoRA step").

  --part kernel   ops.lora_wgrad (csrc/lora.hip) against the path the same product took before it existed: two lmx_op_transpose + lmx_op_gemm (the small operand
                  padded to the GEMM's tile where needed is that path's own business).  rows = 16 x 2048, F in {4096, 11008}, R = 128, both output orientations.
                  The two are timed in alternating rounds in one process; each figure is the median of the rounds with the min .. max spread next to it.
  --part dropout  the LoRA dropout kernels that mask in registers against the materialising path they replace, rows = 16 x 2048, Rp = R = 128, p = 0.05:
                  ops.lora_down_dropout (G adapters sharing x) against G x (ops.dropout + ops.gemm), and ops.lora_wgrad_dropout against ops.dropout +
                  ops.lora_wgrad; alternating rounds, median and min .. max as for --part kernel
  --part lora     one LoRA step (r = 128, alpha = 256, every decoder linear) of the LLaVA-1.5-7B geometry on 4 x 2048 positions, peak allocated bytes;
                  --lora_dropout P runs it with peft's lora_dropout (the reference's scripts: 0.05), 0 = the step without it
  --part full     the full fine-tune step on the same batch (what bench.py --workload config5 runs), peak allocated bytes
Every timing is device events around `reps` back-to-back calls after a warm-up of the same shape; one JSON line per figure."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3           # microseconds per call


def part_kernel(a):
    from llava_mi355x import ops
    dev = torch.device("cuda:0")
    rows, R = a.rows, a.rank
    for F in (4096, 11008):
        big = (torch.randn((rows, F), device=dev) * 0.1).to(torch.bfloat16)
        small = (torch.randn((rows, R), device=dev) * 0.1).to(torch.bfloat16)
        for transposed in (False, True):
            out = torch.empty((R, F) if transposed else (F, R), dtype=torch.bfloat16, device=dev)
            old_out = torch.empty_like(out)
            new = lambda: ops.lora_wgrad(big, small, out, transposed=transposed)
            if transposed:        # out [R, F] = small^T big
                old = lambda: ops.gemm(ops.transpose_padded(small, 64), ops.transpose_padded(big, 64), out=old_out)
            else:                 # out [F, R] = big^T small
                old = lambda: ops.gemm(ops.transpose_padded(big, 64), ops.transpose_padded(small, 64), out=old_out)
            t_new, t_old = [], []
            for _ in range(a.rounds):
                t_new.append(timed(new, a.reps)); t_old.append(timed(old, a.reps))
            ref = (small.double().t() @ big.double()) if transposed else (big.double().t() @ small.double())
            scale = float(ref.abs().max())
            bytes_min = 2.0 * rows * (F + R) + 2.0 * F * R
            med = statistics.median(t_new)
            print(json.dumps({"part": "kernel", "rows": rows, "F": F, "R": R, "transposed": transposed,
                              "lora_wgrad_us": {"median": round(med, 1), "min": round(min(t_new), 1), "max": round(max(t_new), 1)},
                              "transposes_plus_gemm_us": {"median": round(statistics.median(t_old), 1), "min": round(min(t_old), 1), "max": round(max(t_old), 1)},
                              "speedup_of_medians": round(statistics.median(t_old) / med, 2), "lora_wgrad_GBs_of_minimal_traffic": round(bytes_min / med / 1e3, 1),
                              "max_err_new_over_max_ref": float((out.double() - ref).abs().max()) / scale,
                              "max_err_old_over_max_ref": float((old_out.double() - ref).abs().max()) / scale}), flush=True)
        del big, small


def part_dropout(a):
    from llava_mi355x import ops
    dev = torch.device("cuda:0")
    rows, R, p, seed = a.rows, a.rank, 0.05, 1234
    stat = lambda t: {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
    for K, G in ((4096, 3), (4096, 2), (4096, 1), (11008, 1)):
        x = (torch.randn((rows, K), device=dev) * 0.1).to(torch.bfloat16)
        A = (torch.randn((G * R, K), device=dev) * 0.02).to(torch.bfloat16)
        u, u_old = torch.empty((rows, G * R), dtype=torch.bfloat16, device=dev), torch.empty((rows, G * R), dtype=torch.bfloat16, device=dev)
        du = (torch.randn((rows, R), device=dev) * 0.1).to(torch.bfloat16)
        dA, dA_old = torch.empty((R, K), dtype=torch.bfloat16, device=dev), torch.empty((R, K), dtype=torch.bfloat16, device=dev)
        new = lambda: ops.lora_down_dropout(x, A, G, p, seed, 0, 8, out=u)
        def old():
            for g in range(G):
                ops.gemm(ops.dropout(x, p, seed, 0, 8 + g), A[g * R:(g + 1) * R], out=u_old[:, g * R:(g + 1) * R])
        t_new, t_old = [], []
        for _ in range(a.rounds):
            t_new.append(timed(new, a.reps)); t_old.append(timed(old, a.reps))
        scale = float(u_old.float().abs().max())
        print(json.dumps({"part": "dropout", "kernel": "lora_down_dropout", "rows": rows, "K": K, "Rp": R, "G": G, "fused_us": stat(t_new),
                          "dropout_plus_gemm_us": stat(t_old), "speedup_of_medians": round(statistics.median(t_old) / statistics.median(t_new), 2),
                          "max_diff_over_max": float((u.float() - u_old.float()).abs().max()) / scale}), flush=True)
        if G == 1:
            new = lambda: ops.lora_wgrad_dropout(x, du, p, seed, 0, 8, out=dA, transposed=True)
            old = lambda: ops.lora_wgrad(ops.dropout(x, p, seed, 0, 8), du, dA_old, transposed=True)
            t_new, t_old = [], []
            for _ in range(a.rounds):
                t_new.append(timed(new, a.reps)); t_old.append(timed(old, a.reps))
            print(json.dumps({"part": "dropout", "kernel": "lora_wgrad_dropout", "rows": rows, "F": K, "R": R, "fused_us": stat(t_new),
                              "dropout_plus_lora_wgrad_us": stat(t_old), "speedup_of_medians": round(statistics.median(t_old) / statistics.median(t_new), 2),
                              "bits_equal": bool(torch.equal(dA, dA_old))}), flush=True)
        del x, A, u, u_old, du, dA, dA_old


def part_step(a, lora_on):
    from llava_mi355x.train import LoraConfig, TrainStep
    from synthetic import build as harness, recipes as synth
    dev = torch.device("cuda:0")
    cfg = synth.CONFIGS[a.model]
    lc, _ = harness.hf_configs(cfg)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    shapes = synth.tensor_shapes(cfg)
    weights = {k: harness._device_tensor(cfg, k, shapes[k], gen, dev).to(torch.bfloat16) for k in shapes if not k.startswith("vision.") and "vision_tower" not in k}
    torch.cuda.reset_peak_memory_stats(dev)
    ts = TrainStep(lc, weights, dtype=torch.bfloat16, device=dev, lr=2e-5 if not lora_on else 2e-4, weight_decay=0.0, max_grad_norm=1.0, checkpoint=True,
                   max_positions=max(2048, a.seq), lora=LoraConfig(r=a.rank, alpha=2 * a.rank, dropout=a.lora_dropout) if lora_on else None,
                   lr_for=(lambda n: 2e-5 if "mm_projector" in n else 2e-4) if lora_on else None)
    del weights
    torch.cuda.empty_cache()
    B, T = a.batch, a.seq
    L = T - cfg.tokens_per_image + 1
    ids = torch.stack([torch.from_numpy(synth.make_prompt(cfg, L, image_positions=(35,), seed=60 + i)) for i in range(B)])
    labels = ids.clone(); labels[:, :64] = -100; labels[ids == -200] = -100
    feats = (torch.randn((B, cfg.tokens_per_image, lc.mm_hidden_size), device=dev, generator=gen) * 0.5).to(torch.bfloat16)     # stands for the frozen tower's output
    step = lambda: ts.step(ids, labels, None, image_features=feats)
    losses = [float(step()[0].item())]
    peak = torch.cuda.max_memory_allocated(dev)
    free_b, total_b = torch.cuda.mem_get_info(dev)
    ts.keep_budget_bytes = max(0, int(0.88 * total_b) - peak)            # bench.py's rule: keep as many layers' activations as 88 % of the device holds
    for _ in range(a.warmup):
        losses.append(float(step()[0].item()))
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); loss, _ = step(); e1.record(); torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    losses.append(float(loss.item()))
    print(json.dumps({"part": "lora" if lora_on else "full", "model": a.model, "positions": B * T, "rank": a.rank if lora_on else None,
                      "lora_dropout": a.lora_dropout if lora_on else None,
                      "step_ms": {"median": round(statistics.median(times), 1), "min": round(min(times), 1), "max": round(max(times), 1)},
                      "tokens_per_s": round(B * T / statistics.median(times) * 1e3, 1), "kept_layers": ts.last_kept_layers,
                      "peak_allocated_GB_recomputing_step": round(peak / 1e9, 2), "peak_allocated_GB": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2),
                      "flat_elements": ts.part.total, "losses": [round(l, 4) for l in losses]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernel", "dropout", "lora", "full"], required=True)
    ap.add_argument("--rows", type=int, default=16 * 2048)
    ap.add_argument("--rank", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--model", default="llava15_7b")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--lora_dropout", type=float, default=0.0)
    a = ap.parse_args()
    if a.part == "kernel":
        part_kernel(a)
    elif a.part == "dropout":
        part_dropout(a)
    else:
        part_step(a, a.part == "lora")


if __name__ == "__main__":
    main()
