#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X LLaVA forward path (BASELINE.json metric).

Workload (BASELINE.json configs[1]; name in `config.workload`): LLaVA-1.5-7B geometry, bf16, one synthetic 336x336
image + 512-token prompt (one <image> marker -> 1087 positions), greedy 128-token generation.  Random-init weights
(HF init, std 0.02 — no checkpoints exist offline), synthetic inputs, already resident in HBM when timing starts.

One "step" = one whole request through the hot path: encode_images (CLIP ViT-L/14-336, 23 layers, + mlp2x_gelu
projector) -> splice -> decoder prefill (1087 positions) -> 127 decode steps with the KV cache (+ the prefill's pick
= 128 generated tokens).  `value` = generated tokens / wall second over the timed steps, whole job.

  python bench.py --gpus N --steps K --warmup W        (N > 1: launched by torch.distributed.run, one rank per GPU, the decoder tensor-parallel over RCCL /
                                                        the peer-to-peer kernels.  `value` = the WEAK-scaling job: N requests, one per GPU (own image, own prompt), as
                                                        ONE TP = N job — image tower data parallel over the ranks, packed prefill, N sequences decoding together —
                                                        generated tokens of all N requests / wall second; `strong_single_request` = one request over TP = N (the
                                                        latency view), `replicas` = N independent one-GPU replicas, both in the same line.  DESIGN.md §4 "Multi-GPU")
`--dump-outputs DIR` writes the ids the last timed step returned to DIR/output_ids.npy (inputs are seeded: two builds compare output for output).
Extra objects on the JSON line, with `--full` only (measured in the same process after the timed region, HIP events on the launch stream; null without it):
  roofline          dominant kernel of the step by time = decode weight-streaming GEMV family (HBM-bound)
  roofline_prefill  dominant prefill kernel = MFMA GEMM family (MFMA-bound; north_star's 40 % target)
  cpu_baseline      kind "reference": the reference's OWN model files (byte code in oracle/_ref, oracle/ref_shim.py) run on this box's host cores on a bounded
                    sample of the same request; `port` inside it = the CPU oracle restatement (oracle/llava_oracle.py) beside it.  Without oracle/_ref: the port alone.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0     # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0         # MI355X HBM3E spec


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="llava15_7b")
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-batch", action="store_true", help="skip the serving_batch (continuous batching) measurement")
    ap.add_argument("--no-replicas", action="store_true", help="N>1: skip the independent-replicas (data-parallel serving) measurement")
    ap.add_argument("--no-weak", action="store_true", help="N>1: skip the weak-scaling job (N requests as one TP = N job); `value` is then the single request over TP = N (strong)")
    ap.add_argument("--cpu-layers", type=int, default=0, help="0 = time the WHOLE model on the host cores (default); n > 0 = bounded sample of n "
                    "decoder layers, scaled (labelled `extrapolated`; fallback for hosts with too little memory)")
    ap.add_argument("--no-cpu-reference", action="store_true", help="skip the cpu_baseline leg of kind 'reference' (the reference's own model files, sourceless from oracle/_ref)")
    ap.add_argument("--no-cpu-fp32", action="store_true", help="skip the fp32 prefill of the CPU baseline (the parity dtype; layer-streamed upcast, ~20 s)")
    ap.add_argument("--cpu-decode-steps", type=int, default=0, help="decode steps the CPU baseline really runs (0 = all new_tokens - 1; fewer: the rest is priced and the line says so)")
    ap.add_argument("--no-tp-projection", action="store_true", help="skip the tensor-parallel projection (rank-local shards of TP 2 / 4 / 8 timed on this GPU + link model)")
    ap.add_argument("--gemm-variant", type=int, default=0)
    ap.add_argument("--train-batch", type=int, default=1, help="config5: samples per rank and step (the reference uses 16)")
    ap.add_argument("--train-attn-streams", type=int, default=4, help="config5: side streams the per-sample attention launches of a layer spread over (0: one stream)")
    ap.add_argument("--train-keep-gb", type=float, default=-1.0, help="config5: bytes of layer activations kept instead of recomputed (GB; < 0 = what 88 %% of the device "
                                                                      "memory leaves after a fully recomputing step, 0 = recompute every layer as the reference's gradient_checkpointing)")
    ap.add_argument("--train-seq", type=int, default=1024, help="config5: positions per sample after the image splice (the reference caps at 2048)")
    ap.add_argument("--workload", default="config2", choices=["config2", "config3", "config5"],
                    help="config2 (default, BASELINE metric): one request, batch 1.  config3: LLaVA-1.5-13B geometry, 8 requests (8 images), "
                         "chunked prefill (512 rows), the 8 sequences decode together; prefill and decode reported separately.  config5: one "
                         "visual-instruction-tuning step (forward, backward, AdamW, ZeRO-2 over the ranks) of LLaVA-1.5-7B geometry")
    ap.add_argument("--no-parity-probe", action="store_true", help="skip the live parity probe (the fp32 verification engine on the same bf16-rounded weights: "
                                                                  "last-position prefill logits and the first greedy ids of the timed request)")
    ap.add_argument("--no-pmc", action="store_true", help="skip the rocprofv3 --pmc passes that measure roofline.traffic")
    ap.add_argument("--full", action="store_true", help="config2: after the timed steps also measure everything beside the headline (phase split, in-situ kernel profile and "
                                                        "rooflines, live PMC traffic, serving batch, live parity probe, TP projection, CPU baseline; N > 1: replicas). "
                                                        "Without it a run sets up, warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path returned in its last timed step to DIR/<name>.npy "
                                                                        "(integers as float64, floats as float32; at most 64 MB)")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy per array; integer ids as float64 (exact), everything else as float32.  The inputs are seeded, so two builds
    run with the same arguments can be compared output for output."""
    import numpy as np
    out = {k: (v.detach().float() if v.is_floating_point() else v.detach().double()).cpu().numpy() for k, v in arrays.items()}
    total = sum(x.nbytes for x in out.values())
    assert total <= DUMP_LIMIT_BYTES, f"outputs of {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte dump limit"
    os.makedirs(path, exist_ok=True)
    for k, x in out.items():
        np.save(os.path.join(path, k + ".npy"), x)


def flops_prefill(cfg, T, n_images):
    H, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    lin = 2.0 * T * L * (4 * H * H + 3 * H * I)
    attn = 2.0 * T * T * H * L                       # causal: QK^T + PV over the lower triangle
    head = 2.0 * H * cfg.vocab_size
    Dv, Fv, Tv, P = cfg.v_hidden_size, cfg.v_intermediate_size, cfg.num_patches + 1, cfg.num_patches
    n_hs = cfg.v_num_hidden_layers + 1
    v_run = cfg.mm_vision_select_layer % n_hs
    vis = v_run * (2.0 * Tv * (4 * Dv * Dv + 2 * Dv * Fv) + 4.0 * Tv * Tv * Dv) + 2.0 * P * 3 * cfg.v_patch_size ** 2 * Dv
    proj = 2.0 * P * (Dv * H + H * H)
    return dict(linear=lin, attention=attn, lm_head=head, vision=n_images * vis, projector=n_images * proj,
                total=lin + attn + head + n_images * (vis + proj))


def usable_cores() -> int:
    """Cores this process may really use: affinity mask, clipped by the cgroup CPU quota (containers often expose every
    host CPU in os.cpu_count() while being limited to a few)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            n = min(n, max(1, int(float(q[0]) / float(q[1]))))
    except Exception:  # noqa: BLE001
        try:
            quota = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); period = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if quota > 0:
                n = min(n, max(1, quota // period))
        except Exception:  # noqa: BLE001
            pass
    return n


def _cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:  # noqa: BLE001
        pass
    return "unknown"


def _host_weights(cfg, dt):
    """HF-init weights of the whole model on the host, one tensor at a time (peak = the bf16 model + one fp32 tensor)."""
    from synthetic import recipes as synth
    g = torch.Generator().manual_seed(0)
    w = {}
    for name, shp in synth.tensor_shapes(cfg).items():
        if name.endswith("norm.weight") or ("layer_norm" in name and name.endswith(".weight")) or name.endswith("pre_layrnorm.weight"):
            w[name] = torch.ones(shp, dtype=dt)
        elif name.endswith(".bias"):
            w[name] = torch.zeros(shp, dtype=dt)
        else:
            w[name] = (torch.randn(shp, generator=g) * 0.02).to(dt)
    return w


def cpu_baseline_full(cfg, ids, pix, new_tokens, with_fp32, decode_steps=0, prefill_runs=3):
    """The same request through the CPU oracle (oracle/llava_oracle.py, torch CPU) on this box's host cores — the WHOLE model, measured:
    prefill = encode_images + splice + all decoder layers + last-row lm_head, median of 3 after 1 warm-up; decode = the request's
    real greedy steps with the KV cache (all new_tokens - 1 of them by default; with fewer the remainder is priced at the measured mean and
    the result carries `partly_priced`)."""
    from oracle import llava_oracle as O
    torch.set_num_threads(usable_cores())
    w = _host_weights(cfg, torch.bfloat16)
    ids_c, pix_c = ids.cpu(), pix.cpu().to(torch.bfloat16)
    n_dec = new_tokens - 1 if decode_steps <= 0 else min(decode_steps, new_tokens - 1)
    with torch.no_grad():
        def prefill():
            t0 = time.perf_counter()
            logits, past, _, _ = O.llava_forward(w, cfg, ids_c, pix_c, last_only=True)
            return time.perf_counter() - t0, logits, past
        prefill()                                   # warm-up
        runs = [prefill() for _ in range(max(1, prefill_runs))]
        t_pre = sorted(r[0] for r in runs)[len(runs) // 2]
        logits, past = runs[-1][1], runs[-1][2]
        T = past[0][0].shape[2]
        t0 = time.perf_counter()
        toks = []
        for _ in range(n_dec):
            tok = int(torch.argmax(logits[0, -1].float()))
            toks.append(tok)
            logits, past = O.llama_forward(w, cfg, w["model.embed_tokens.weight"][torch.tensor([[tok]])], past=past, last_only=True)
        t_dec = (time.perf_counter() - t0) / n_dec
        del past
        fp32 = None
        if with_fp32:
            # one fp32 prefill with the same (bf16-representable) weights, upcast layer by layer (27 GB of fp32 weights never resident)
            import torch.nn.functional as F
            t0 = time.perf_counter()
            small = {k: v.float() for k, v in w.items() if not k.startswith("model.layers.") and k != "lm_head.weight"}
            _, _, _, _, emb, _ = O.prepare_inputs_labels_for_multimodal(small, cfg, ids_c, None, None, None, None, pix_c.float())
            Tn = emb.shape[1]
            cos, sin = O.rope_cos_sin(cfg, torch.arange(Tn)[None], torch.float32)
            qi = torch.arange(Tn)[:, None]; ki = torch.arange(Tn)[None, :]
            bias = torch.zeros((1, 1, Tn, Tn)).masked_fill(~(ki <= qi)[None, None], torch.finfo(torch.float32).min)
            h = emb
            for i in range(cfg.num_hidden_layers):
                pfx = f"model.layers.{i}."
                h, _ = O.decoder_layer({k: v.float() for k, v in w.items() if k.startswith(pfx)}, cfg, i, h, cos, sin, None, bias)
            F.linear(O.rms_norm(h[:, -1:], small["model.norm.weight"], cfg.rms_norm_eps), w["lm_head.weight"].float())
            fp32 = {"prefill_ms": (time.perf_counter() - t0) * 1e3, "note": "one run, includes the per-layer bf16->fp32 weight upcast"}
    step_s = t_pre + (new_tokens - 1) * t_dec
    return {"value": new_tokens / step_s, "unit": "generated tokens/s", "cores": torch.get_num_threads(), "cpu": _cpu_model_name(), "kind": "port",
            "dtype": "bf16", "measured": "whole model", "prefill_ms": t_pre * 1e3, "prefill_runs_ms": [r[0] * 1e3 for r in runs],
            "decode_tokens_per_s": 1.0 / t_dec, "decode_steps_timed": n_dec, "decode_steps_priced": new_tokens - 1 - n_dec,
            "partly_priced": n_dec < new_tokens - 1, "first_ids": toks[:4], "fp32": fp32,
            "sample": f"the whole request on the host: CLIP tower + projector + splice + {cfg.num_hidden_layers} decoder layers at T={T} "
                      f"(median of {len(runs)} prefill(s) after a warm-up) + {n_dec} real greedy decode steps with the KV cache"
                      + ("" if n_dec == new_tokens - 1 else f"; the remaining {new_tokens - 1 - n_dec} steps of the request priced at the measured per-step time")}


def cpu_baseline_reference(cfg, ids, pix, new_tokens, decode_steps=0):
    """kind "reference": the REFERENCE'S OWN model code on this box's host cores — llava/model/llava_arch.py, language_model/llava_llama.py,
    multimodal_encoder/clip_encoder.py, multimodal_projector/builder.py over the installed transformers, imported sourceless from oracle/_ref/llava_pyc (byte code
    of /root/reference built by oracle/build_ref_worker.py; in the build container the tree itself) through oracle/ref_shim.py.  bf16 (the GPU path's dtype),
    eager attention, the same request with the same HF-init weights.  Bounded sample: the worker's call `model.generate(inputs, images=..., do_sample=False)`
    (llava/serve/model_worker.py:174-185) once for 1 new token (= image encode + splice + prefill + the first pick; run twice, second taken) and once for
    1 + decode_steps tokens; per-step decode time = the difference / decode_steps, the rest of the request is priced at it.  None when the files are absent."""
    from oracle import ref_shim
    if not ref_shim.available():
        return None
    torch.set_num_threads(usable_cores())
    t0 = time.perf_counter()
    w = _host_weights(cfg, torch.bfloat16)
    model = ref_shim.build_reference_model(cfg, w, dtype=torch.bfloat16, fast_init=True)
    del w
    build_s = time.perf_counter() - t0
    ids_c, pix_c = ids.cpu(), pix.cpu().to(torch.bfloat16)
    n_dec = max(1, min(decode_steps if decode_steps > 0 else new_tokens - 1, new_tokens - 1))      # default: every decode step of the request is timed

    def gen(n):
        t = time.perf_counter()
        with torch.no_grad():
            out = model.generate(inputs=ids_c, images=pix_c, do_sample=False, max_new_tokens=n, use_cache=True, past_key_values=ref_shim.subscriptable_cache())
        return time.perf_counter() - t, out[0, ids_c.shape[1]:].tolist()
    gen(1)
    t1, first = gen(1)
    t2, toks = gen(1 + n_dec)
    t_dec = max(t2 - t1, 1e-9) / n_dec
    step_s = t1 + (new_tokens - 1) * t_dec
    import transformers
    return {"value": new_tokens / step_s, "unit": "generated tokens/s", "cores": torch.get_num_threads(), "cpu": _cpu_model_name(), "kind": "reference",
            "dtype": "bf16", "measured": "whole model, the reference's own forward + HF greedy loop", "prefill_ms": t1 * 1e3,
            "decode_tokens_per_s": 1.0 / t_dec, "decode_steps_timed": n_dec, "decode_steps_priced": new_tokens - 1 - n_dec, "partly_priced": n_dec < new_tokens - 1,
            "first_ids": toks[:4], "model_build_s": build_s, "transformers": transformers.__version__, "sourceless": ref_shim.is_sourceless(),
            "sample": f"LlavaLlamaForCausalLM.generate of the reference's own files (bf16, eager attention) on the host: 1 new token (tower + projector + splice + "
                      f"{cfg.num_hidden_layers} decoder layers + pick; second of two runs) and {1 + n_dec} new tokens; decode step = the difference / {n_dec}; "
                      f"the other {new_tokens - 1 - n_dec} steps of the request priced at it"}


def parity_record(model_name):
    """What the parity gate asserts for the kernels this line times, with the figures of the latest committed run of tests/test_full_depth_gpu.py
    (profiles/r0N_full_depth_*.json; NOT re-measured by the bench: the fp32 oracle pass over 7B takes minutes of host time).  Every report carries the hash of the
    kernel sources it was measured on (synthetic/treehash.py); `stale` says whether that is the tree this bench runs on — after a kernel change the committed
    figures are the previous build's until the suite has been re-run and its reports committed."""
    from synthetic.treehash import csrc_sha16
    here = csrc_sha16()
    out = {"asserted": {"fp32_engine_vs_fp32_oracle": "logits of all 1087 positions max-abs-err <= 1e-3 (north_star tolerance), 32 greedy ids identical, full depth",
                        "bf16_engine_vs_fp32_oracle": "max and rms error of image features and last-position logits <= 1.25 x the reference's own bf16 pass + 1 ulp; "
                                                      "every greedy id within the combined bf16 noise of the bf16 oracle's maximum",
                        "integers": "image-token rows, attention_mask, position_ids, labels bit-exact (tests/test_model_gpu.py, goldens of the reference's own code)",
                        "goldens_made_with": "transformers 5.15 (the reference pins 4.31: fp32 semantics identical, CLIP softmax precision differs — SURVEY 7)"},
           "source": "tests/test_full_depth_gpu.py, committed run under profiles/ (not re-measured here)", "csrc_sha16_of_this_run": here}

    def latest(stem):
        for rnd in ("r06", "r05"):
            p = os.path.join(ROOT, "profiles", f"{rnd}_{stem}.json")
            if os.path.exists(p):
                with open(p) as f:
                    return json.load(f), os.path.basename(p)
        return None, None
    stamps = []
    try:
        rep, name = latest("full_depth_fp32_llava15_7b")
        r = rep["fp32_full_depth_T1087"]
        out["fp32_max_abs"] = r.get("logits_max_abs_err_all_positions", r.get("logits_max_abs_err"))
        out["fp32_positions_compared"] = r.get("positions_compared", 1)
        out["fp32_greedy_ids_identical"] = [r.get("greedy_ids_identical"), r.get("greedy_ids_compared")]
        out["fp32_report"] = name
        stamps.append(rep.get("csrc_sha16"))
    except Exception:  # noqa: BLE001
        pass
    try:
        r, name = latest(f"full_depth_{model_name}")
        out["bf16_logits_err_of_max_logit"] = r["logits"]["engine"]
        out["ref_bf16_logits_err_of_max_logit"] = r["logits"]["hf_bf16"]
        out["bf16_vs_ref_bf16_ratio"] = r["logits"]["engine"] / r["logits"]["hf_bf16"]
        out["bf16_greedy_ids_identical_to_bf16_oracle"] = [r["greedy"]["identical"], len(r["greedy"]["steps"])]
        out["bf16_report"] = name
        stamps.append(r.get("csrc_sha16"))
    except Exception:  # noqa: BLE001
        pass
    out["reports_csrc_sha16"] = stamps
    out["stale"] = not stamps or any(st != here for st in stamps)      # True: the figures above were measured on other kernel sources than this run's
    return out


def cpu_baseline(cfg, T, new_tokens, n_layers):
    """FALLBACK (--cpu-layers n): bounded sample on the host cores through the CPU oracle (torch CPU), in fp32 and bf16:
    full CLIP tower + projector for 1 image, `n_layers` real-geometry decoder layers of prefill at T positions and of
    4 decode steps at ctx T; decoder time scaled by L / n_layers, lm_head timed once: EXTRAPOLATED, labelled so."""
    from oracle import llava_oracle as O
    from synthetic import recipes as synth
    torch.set_num_threads(usable_cores())
    small = synth.with_layers(cfg, n_layers)
    g = torch.Generator().manual_seed(0)
    w32 = {}
    for name, shp in synth.tensor_shapes(small).items():
        if name.endswith("norm.weight") or ("layer_norm" in name and name.endswith(".weight")) or name.endswith("pre_layrnorm.weight"):
            w32[name] = torch.ones(shp)
        elif name.endswith(".bias"):
            w32[name] = torch.zeros(shp)
        else:
            w32[name] = torch.randn(shp, generator=g) * 0.02
    pix32 = torch.from_numpy(synth.make_pixels(cfg, 1))
    emb32 = torch.randn((1, T, cfg.hidden_size), generator=g) * 0.02
    scale = cfg.num_hidden_layers / n_layers
    nd = 4
    per = {}
    for dname, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        if per and per["fp32"]["sample_wall_s"] > 15.0:
            break                                        # keep the whole bench within a few minutes on slow hosts
        w = {k: v.to(dt) for k, v in w32.items()}
        pix, emb = pix32.to(dt), emb32.to(dt)
        with torch.no_grad():
            t0 = time.perf_counter(); O.encode_images(w, small, pix); t_vis = time.perf_counter() - t0
            t0 = time.perf_counter(); _, past = O.llama_forward(w, small, emb, last_only=True); t_pre = time.perf_counter() - t0
            tok = emb[:, :1]
            t0 = time.perf_counter()
            for _ in range(nd):
                _, past = O.llama_forward(w, small, tok, past=past, last_only=True)
            t_dec = (time.perf_counter() - t0) / nd
            h = emb[:, -1:]
            t0 = time.perf_counter(); O.rms_norm(h, w["model.norm.weight"], cfg.rms_norm_eps) @ w["lm_head.weight"].t(); t_head = time.perf_counter() - t0
        prefill_s = t_vis + max(t_pre - t_head, 0.0) * scale + t_head
        decode_s = max(t_dec - t_head, 0.0) * scale + t_head
        step_s = prefill_s + (new_tokens - 1) * decode_s
        per[dname] = {"tokens_per_s": new_tokens / step_s, "prefill_ms": prefill_s * 1e3, "decode_tokens_per_s": 1.0 / decode_s,
                      "sample_wall_s": t_vis + t_pre + nd * t_dec + t_head}
    best = max(per, key=lambda k: per[k]["tokens_per_s"])
    return {"value": per[best]["tokens_per_s"], "unit": "generated tokens/s", "cores": torch.get_num_threads(), "cpu": _cpu_model_name(), "kind": "port",
            "measured": "extrapolated", "dtype": best, "prefill_ms": per[best]["prefill_ms"], "decode_tokens_per_s": per[best]["decode_tokens_per_s"], "by_dtype": per,
            "sample": f"EXTRAPOLATED: full CLIP tower+projector (1 image) + {n_layers}/{cfg.num_hidden_layers} decoder layers at real geometry: "
                      f"prefill T={T} and {nd} decode steps at ctx {T}; decoder time scaled x{scale:g}, lm_head timed once"}


def tp_projection(cfg, dtype, dev, ids, pix, new_tokens, worlds=(2, 4, 8), batch=32):
    """What the request and a serving batch should look like at TP = 2 / 4 / 8 — a PROJECTION, printed so that the first real multi-GPU run has a prediction to be
    judged against (no multi-GPU node was available to the builder).  Measured part: ONE engine instance holds rank 0's shard of a TP = W group (the
    production shard selection of Model::load_weight: the rank-local GEMM / GEMV / attention shapes are the real ones) and the all-reduce is replaced
    through lmx_tp_set_allreduce_hook by a no-op that counts calls, so the timed sections are the rank's compute incl. every launch boundary:
      rank_compute_prefill_ms           the WHOLE prefill as a rank runs it: replicated CLIP tower + projector + splice (not sharded) and the sharded decoder,
                                        chunk as one piece (the two-half pipeline is for the RCCL ring; with the two-shot all-reduce it only costs GEMM efficiency)
      rank_compute_decode_ms_per_token  batch-1 decode
      serving_batch                     `batch` sequences at the request's context stepping together (lmx_decode_batch on the shard)
    Modelled part: the all-reduces, two ways.  `p2p` = this repo's own kernels (csrc/p2p.hip): decode-sized rows through the one-shot kernel (6.3 us per
    launch measured between two processes on one GPU + one xGMI hop taken as 2 us + rows x H x 2 B / link), prefill-sized messages through the two-shot
    reduce-scatter + all-gather kernel from 4 ranks on (2 phases x message / W per link at 153 GB/s, W - 1 links busy at once, + the kernel's own cost measured at
    the real message size between two processes on one GPU: 49 us + 0.036 us per row), RCCL's ring at 2 ranks.
    weak                              W requests — one per GPU — as ONE job on the shard (model.generate_batch: tower data parallel over the images, packed prefill,
                                      W sequences decoding together), its all-reduces priced message by message as the engine issued them; `measured_tp1.same_jobs_on_one_gpu`
                                      holds the same jobs really run on this one GPU (batching alone)
    `ring` = RCCL's ring over point-to-point xGMI (2 (W - 1) / W x message over one link + 12 us), the fallback when the exchange buffers cannot be mapped.
    No overlap is credited in either.  Batch-1 latency cannot scale: a token is 2 L + 1 dependent all-reduces and ~160 dependent launches whatever W is;
    the tower is replicated.  What scales is the weight stream, i.e. the serving batch — that is the workload the >= 6x claim is about."""
    import ctypes
    from llava_mi355x import _C
    from llava_mi355x.batching import DecodeBatch
    from llava_mi355x.model import LmxKVCache
    from synthetic import build as harness
    HOOK_T = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p)
    H, L, V = cfg.hidden_size, cfg.num_hidden_layers, cfg.vocab_size
    T = ids.shape[1] - 1 + cfg.tokens_per_image
    es = 2
    # two-shot kernel, measured between two processes on ONE MI355X at the real width (tests/test_tp_p2p_gpu.py::test_two_shot_allreduce_real_width, 64 workgroups per
    # rank, profiles/r04_p2p_big_wgs.txt): 88 us for 1087 x 4096 and 104 us for 1536 x 4096 bf16 -> 49 us of protocol + 0.036 us per row of local traffic (both ranks'
    # copies on one chip: pessimistic for a node, where each rank has its own HBM) — the wire time of the node comes on top.  From 4 ranks on; at 2 ranks the engine
    # keeps RCCL for these messages (engine.h: p2p_big_usable), modelled as the ring.
    link_gbs, ring_lat_us, oneshot_us, twoshot_lat_us, twoshot_us_per_row = 153.0, 12.0, 6.3 + 2.0, 49.0, 0.036 * H / 4096.0
    out = {"what": "projection: rank-local compute measured on this GPU (rank 0's shard, no-op all-reduce) + modelled all-reduces; NOT a multi-GPU measurement",
           "link_model": {"xgmi_link_GBps": link_gbs, "rccl_ring_latency_us": ring_lat_us, "p2p_oneshot_us": oneshot_us, "p2p_twoshot_latency_us": twoshot_lat_us,
                          "p2p_twoshot_us_per_row": twoshot_us_per_row,
                          "p2p": "decode rows: one-shot kernel (latency + rows x H x 2 B / link); prefill-sized messages at W >= 4: two-shot reduce-scatter + all-gather "
                                 "(measured protocol + per-row local traffic of the kernel on one GPU + 2 x message / W / link), csrc/p2p.hip; at W = 2 they stay on RCCL (ring model)",
                          "ring": "2 (W - 1) / W x message / link + latency per all-reduce (RCCL fallback)", "overlap_credited": False},
           "by_world": {}}
    old_overlap = os.environ.get("LMX_TP_OVERLAP")
    os.environ["LMX_TP_OVERLAP"] = "0"                     # chunk as one piece (see the docstring)
    try:
        for W in worlds:
            if cfg.num_attention_heads % W or cfg.num_key_value_heads % W:
                continue
            calls = {"n": 0, "sizes": []}

            def hook(buf, count, dtype_code, stream, ctx):
                calls["n"] += 1
                calls["sizes"].append(int(count))
            m = harness.build_model(cfg, dtype=dtype, seed=0, device_rng=True, device=dev, tp_rank=0, tp_world=W, max_position=2048)
            hk = HOOK_T(hook); m._hook_keepalive = hk
            # two stand-ins for the all-reduce: the python callback COUNTS (calls, message sizes; run once, untimed) — it costs 10 - 20 us of host time per call,
            # which at 65 calls per decode step would be most of a TP = 8 step — and a C function that does nothing (libc's getpid, its arguments ignored) for
            # every timed pass, so that the timed sections are the rank's own launches only
            counting = ctypes.cast(hk, ctypes.c_void_p)
            silent = ctypes.cast(ctypes.CDLL(None).getpid, ctypes.c_void_p)
            use_hook = lambda fn: _C.check(_C.lib.lmx_tp_set_allreduce_hook(m._h, fn, None))
            use_hook(counting)
            pre, dec, front = [], [], []
            embeds = None
            for r in range(4):
                use_hook(counting if r == 0 else silent)
                c = LmxKVCache(m, 1)
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                torch.cuda.synchronize()
                if r == 0:
                    calls["n"] = 0
                e[0].record()
                _, _, _, _, embeds, _ = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, pix)      # tower + projector + splice: replicated on every rank
                e[1].record()
                _C.check(_C.lib.lmx_prefill(m._h, c.seqs[0], _C.ptr(embeds[0]), embeds.shape[1], 0, None, 0, 1, _C.stream_handle()))
                e[2].record()
                if r == 0:
                    n_pre = calls["n"]
                _C.check(_C.lib.lmx_decode(m._h, c.seqs[0], -1, new_tokens - 1, None, 1, _C.stream_handle()))
                e[3].record(); torch.cuda.synchronize()
                if r:
                    front.append(e[0].elapsed_time(e[1])); pre.append(e[0].elapsed_time(e[2])); dec.append(e[2].elapsed_time(e[3]) / (new_tokens - 1))
                c.close()
            # serving batch on the shard
            caches = []
            for _ in range(batch):
                c = LmxKVCache(m, 1)
                _C.check(_C.lib.lmx_prefill(m._h, c.seqs[0], _C.ptr(embeds[0]), embeds.shape[1], 0, None, 0, 1, _C.stream_handle()))
                caches.append(c)
            bt = DecodeBatch(m, batch)
            seqs = [c.seqs[0] for c in caches]
            bt.step(seqs, None, 2, True, want_ids=False)
            torch.cuda.synchronize()
            eb = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            eb[0].record(); bt.step(seqs, None, 16, True, want_ids=False); eb[1].record()
            torch.cuda.synchronize()
            batch_ms = eb[0].elapsed_time(eb[1]) / 16
            bt.close()
            for c in caches:
                c.close()
            # ---- weak scaling: W requests — one per GPU of the group — as ONE tensor-parallel job on this rank's shard (generate_batch: the tower
            #      data parallel over the images, packed prefill in pieces of W x 512 rows, the W sequences decode together)
            weak_t, weak_sizes = [], []
            prompts_w, images_w = weak_job_inputs(cfg, dev, dtype, W, ids.shape[1])
            for r in range(3):
                use_hook(counting if r == 0 else silent)
                torch.cuda.synchronize()
                if r == 0:
                    calls["sizes"] = []
                t0 = time.perf_counter()
                m.generate_batch(prompts_w, images_w, max_new_tokens=new_tokens, eos_token_id=-1, run_ahead=new_tokens, prefill_chunk=512, capacity=W)
                torch.cuda.synchronize()
                if r:
                    weak_t.append((time.perf_counter() - t0) * 1e3)
                else:
                    weak_sizes = list(calls["sizes"])
            del m
            torch.cuda.empty_cache()
            med = lambda xs: sorted(xs)[len(xs) // 2]
            pre_ms, dec_ms, front_ms = med(pre), med(dec), med(front)
            msg = T * H * es
            n_ar = 2 * L
            ring_us = ring_lat_us + 2.0 * (W - 1) / W * msg / (link_gbs * 1e3)
            two_us = (twoshot_lat_us + twoshot_us_per_row * T + 2.0 * (msg / W) / (link_gbs * 1e3)) if W >= 4 else ring_us
            dec_ar_us = oneshot_us + H * es / (link_gbs * 1e3)
            bat_ar_us = oneshot_us + batch * H * es / (link_gbs * 1e3)
            comm = {"p2p": {"prefill_ms": n_ar * two_us / 1e3, "decode_ms_per_token": (n_ar + 1) * dec_ar_us / 1e3, "batch_step_ms": (n_ar + 1) * bat_ar_us / 1e3},
                    "ring": {"prefill_ms": n_ar * ring_us / 1e3, "decode_ms_per_token": (n_ar + 1) * (ring_lat_us + 2.0 * (W - 1) / W * H * es / (link_gbs * 1e3)) / 1e3,
                             "batch_step_ms": (n_ar + 1) * (ring_lat_us + 2.0 * (W - 1) / W * batch * H * es / (link_gbs * 1e3)) / 1e3}}
            row = {"rank_compute_prefill_ms": pre_ms, "of_which_replicated_tower_and_splice_ms": front_ms, "rank_compute_decode_ms_per_token": dec_ms,
                   "allreduce_calls_prefill": n_pre, "serving_batch": {"batch": batch, "rank_compute_ms_per_step": batch_ms}, "modelled_comm": comm}
            for k, cm in comm.items():
                p_ms, d_ms, b_ms = pre_ms + cm["prefill_ms"], dec_ms + cm["decode_ms_per_token"], batch_ms + cm["batch_step_ms"]
                row[k] = {"projected_prefill_ms": p_ms, "projected_decode_ms_per_token": d_ms,
                          "projected_value_tokens_per_s": new_tokens / ((p_ms + (new_tokens - 1) * d_ms) * 1e-3),
                          "projected_batch_decode_tokens_per_s": batch * 1e3 / b_ms}
            # the weak job's all-reduces, message by message as the engine issued them (the image-feature gather, the prefill pieces, the decode rows)
            def ar_us(count, kind):
                rows_ = (count + H - 1) // H
                if kind == "ring":
                    return ring_lat_us + 2.0 * (W - 1) / W * count * es / (link_gbs * 1e3)
                if rows_ <= 32:
                    return oneshot_us + count * es / (link_gbs * 1e3)
                if W < 4:
                    return ring_lat_us + 2.0 * (W - 1) / W * count * es / (link_gbs * 1e3)
                return twoshot_lat_us + twoshot_us_per_row * rows_ + 2.0 * (count * es / W) / (link_gbs * 1e3)
            wk_ms = min(weak_t)
            wk = {"requests": W, "what": f"{W} requests (own image + own {ids.shape[1]}-token prompt each), one per GPU of the TP = {W} group, as ONE job: tower data parallel over the "
                                         f"images + feature all-gather, packed prefill in pieces of {W} x 512 rows, {W} sequences decoding together (model.generate_batch); "
                                         "host work of the job included",
                  "rank_compute_job_ms": wk_ms, "allreduce_calls": len(weak_sizes), "allreduce_bytes": int(sum(weak_sizes)) * es}
            for kind in ("p2p", "ring"):
                c_ms = sum(ar_us(c, kind) for c in weak_sizes) / 1e3
                wk[kind] = {"modelled_comm_ms": c_ms, "projected_job_ms": wk_ms + c_ms, "projected_value_tokens_per_s": W * new_tokens / ((wk_ms + c_ms) * 1e-3)}
            wk["projected_value_tokens_per_s"] = wk["p2p"]["projected_value_tokens_per_s"]
            row["weak"] = wk
            # the headline columns follow the repo's own all-reduce kernels
            row.update({"projected_prefill_ms": row["p2p"]["projected_prefill_ms"], "projected_decode_ms_per_token": row["p2p"]["projected_decode_ms_per_token"],
                        "projected_value_tokens_per_s": row["p2p"]["projected_value_tokens_per_s"],
                        "modelled_comm_prefill_ms": comm["p2p"]["prefill_ms"], "modelled_comm_decode_ms_per_token": comm["p2p"]["decode_ms_per_token"]})
            out["by_world"][str(W)] = row
    finally:
        if old_overlap is None:
            os.environ.pop("LMX_TP_OVERLAP", None)
        else:
            os.environ["LMX_TP_OVERLAP"] = old_overlap
    return out


def weak_job_inputs(cfg, dev, dtype, n_req, prompt_len):
    """The weak-scaling job's requests: n_req x (own seeded image + own seeded prompt of the headline shape); the same on every rank."""
    from synthetic import recipes as synth
    prompts = [torch.from_numpy(synth.make_prompt(cfg, prompt_len, image_positions=(35,), seed=2 + i))[None].to(dev) for i in range(n_req)]
    images = [torch.from_numpy(synth.make_pixels(cfg, 1, seed=1 + i)).to(dev, dtype) for i in range(n_req)]
    return prompts, images


def calibrate_event_overhead(dev):
    """How much a HIP event pair around ONE launch overstates that kernel's duration: 2 x T(scope with one GEMV) - T(scope with two
    back-to-back GEMVs of the same shape, different weights).  An empty scope measures the marker-to-marker latency (~4.5 us), which is
    more than what the pair adds around a real kernel (part of it overlaps the kernel's own launch); this difference form is what
    brings the in-situ per-launch averages into agreement with rocprofv3's kernel durations."""
    import math
    from llava_mi355x import ops
    N = K = 4096
    ws = [(torch.randn(N, K, device=dev) / math.sqrt(K)).bfloat16() for _ in range(8)]
    x = torch.randn(1, K, device=dev).bfloat16(); out = torch.empty(1, N, device=dev, dtype=torch.bfloat16)
    # scopes are queued back to back and resolved after ONE synchronize, like the engine's in-situ profile (the host runs ahead of the
    # GPU; a synchronize per scope would expose the launch latency of an idle stream and overstate the pair's cost)
    def run(n, reps=120):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for i, (e0, e1) in enumerate(ev):
            e0.record()
            for j in range(n):
                ops.gemv(x, ws[(i + j) % 8], out=out)
            e1.record()
        torch.cuda.synchronize()
        ts = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[20:])
        return ts[len(ts) // 2]
    run(2, 40)
    t1, t2 = run(1), run(2)
    return max(0.0, 2.0 * t1 - t2), t1, t2


def pmc_traffic(root):
    """HBM-side bytes per launch of the decode GEMV family, measured NOW: two rocprofv3 passes (FETCH_SIZE, WRITE_SIZE: separate --pmc
    runs with --kernel-trace only, as MI355X_MICROARCH.md §HBM prescribes) over the cold-cache single-kernel driver tools/mb_gemv_cold.py
    (32 distinct weight matrices per shape; rocprofv3 --pmc does not survive wrapping this whole process).  gfx950 corrections from the
    same section: the counters are KiB, and FETCH_SIZE tallies a wide coalesced stream at half its bytes."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    names = {"qkv": (12288, 4096), "o_proj": (4096, 4096), "gate_up": (22016, 4096), "down": (4096, 11008)}
    sums = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="lmx_pmc_")
        try:
            subprocess.run([exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                            os.path.join(root, "tools", "mb_gemv_cold.py")], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=240,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
            acc, cnt = {}, {}
            for r in csv.DictReader(open(f)):
                if r["Counter_Name"] != ctr or "gemv" not in r["Kernel_Name"]:      # gemv2_kernel (hand-counted stream) or gemv_kernel
                    continue
                key = r.get("Grid_Size", "") + "|" + r["Kernel_Name"].split("(")[0][-24:]      # shapes can share a grid size (o_proj / down_proj): the instantiation tells them apart
                acc[key] = acc.get(key, 0.0) + float(r["Counter_Value"]); cnt[key] = cnt.get(key, 0) + 1
            sums[ctr] = {k: acc[k] / cnt[k] for k in acc}
        except Exception as ex:  # noqa: BLE001
            return {"error": repr(ex)[:200]}
        finally:
            shutil.rmtree(d, ignore_errors=True)
    # launches of one shape share a grid size; pair the grids of the two passes and weight every shape by its launches per token (32 each)
    fetch, write = sums["FETCH_SIZE"], sums["WRITE_SIZE"]
    total = sum((2.0 * fetch[k] + write.get(k, 0.0)) * 1024.0 for k in fetch)
    algo = sum(n * k * 2.0 for n, k in names.values())
    return {"hbm_bytes_per_layer_4_launches": total, "algorithmic_bytes_per_layer": algo, "ratio": total / algo, "by_grid_fetch_KiB": fetch, "by_grid_write_KiB": write}


def pmc_prefill_traffic(root, T, iters=4):
    """HBM-side bytes per launch of the four prefill GEMM shapes, measured NOW: two rocprofv3 passes (FETCH_SIZE, WRITE_SIZE; --pmc with
    --kernel-trace only) over tools/mb_gemm_prefill.py, which launches q|k|v, gate|up, o_proj, down_proj `iters` times each in that order.  Dispatches are told
    apart by kernel instantiation and order: the un-split kernel serves q|k|v then gate|up; the K-sliced kernel + its reduction serve o_proj then down_proj
    (their figure = GEMM + reduction: the fp32 partial tiles are written by one and read by the other).  gfx950 corrections as in pmc_traffic."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    per = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="lmx_pmcp_")
        try:
            subprocess.run([exe, "--pmc", ctr, "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                            os.path.join(root, "tools", "mb_gemm_prefill.py"), str(iters), str(T)], cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=240,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=True)
            f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)[0]
            rows = [r for r in csv.DictReader(open(f)) if r["Counter_Name"] == ctr]
            rows.sort(key=lambda r: int(r.get("Dispatch_Id", 0)))
            # gemm8p_kernel<T, SPLIT>: SPLIT = 1 is the un-split launch (round 5's prune left these two template parameters)
            unsplit = [float(r["Counter_Value"]) for r in rows if "gemm8p_kernel" in r["Kernel_Name"] and ", 1>" in r["Kernel_Name"]]
            sliced = [float(r["Counter_Value"]) for r in rows if "gemm8p_kernel" in r["Kernel_Name"] and ", 1>" not in r["Kernel_Name"]]
            reduce_ = [float(r["Counter_Value"]) for r in rows if "splitk_reduce" in r["Kernel_Name"]]
            if len(unsplit) != 2 * iters or len(sliced) != 2 * iters or len(reduce_) != 2 * iters:
                return {"error": f"unexpected dispatch counts {len(unsplit)} / {len(sliced)} / {len(reduce_)} for {ctr}"}
            mean = lambda xs: sum(xs) / len(xs)
            per[ctr] = {"qkv": mean(unsplit[:iters]), "gate_up": mean(unsplit[iters:]), "o_proj": mean(sliced[:iters]) + mean(reduce_[:iters]),
                        "down": mean(sliced[iters:]) + mean(reduce_[iters:])}
        except Exception as ex:  # noqa: BLE001
            return {"error": repr(ex)[:200]}
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return {k: (2.0 * per["FETCH_SIZE"][k] + per["WRITE_SIZE"][k]) * 1024.0 for k in per["FETCH_SIZE"]}


def run_config5(a, model, cfg, synth, dev, dtype, barrier, world, rank, share, build_s):
    """BASELINE config 5: one visual-instruction-tuning step of LLaVA-1.5-7B geometry (LLM + mm_projector trainable, CLIP tower frozen), AdamW on fp32
    master weights, ZeRO-2 over the data-parallel ranks (one rank = one GPU; N = 1 keeps the whole optimiser state).  A step = frozen tower on the
    rank's images -> packed forward -> backward (activation recompute per layer) -> bucketed reduce-scatter -> clip -> AdamW -> all-gather.
    The backward kernels are parity-first (csrc/train.hip; the attention backward of 16-bit models runs on the matrix cores since round 3, csrc/attn_bwd.hip;
    dgrad / wgrad still transpose their operands onto the forward GEMM): the default micro-batch is small
    (--train-batch 1 --train-seq 1024); the number is a first measurement of a correct step, not a tuned one."""
    import numpy as np
    from synthetic import build as harness
    from llava_mi355x.train import TrainStep
    group = None
    if world > 1:
        import torch.distributed as dist
        group = dist.new_group(backend="gloo") if share else dist.group.WORLD
    lc, _ = harness.hf_configs(cfg)
    gen = torch.Generator(device=dev); gen.manual_seed(0)
    names = [k for k in synth.tensor_shapes(cfg) if not k.startswith("vision.") and "vision_tower" not in k]
    weights = {k: harness._device_tensor(cfg, k, synth.tensor_shapes(cfg)[k], gen, dev).to(dtype) for k in names}
    ts = TrainStep(lc, weights, dtype=dtype, device=dev, lr=2e-5, weight_decay=0.0, max_grad_norm=1.0, group=group, checkpoint=True,
                   max_positions=max(2048, a.train_seq), attn_streams=a.train_attn_streams)
    del weights
    torch.cuda.empty_cache()
    B, T = a.train_batch, a.train_seq
    L = T - cfg.tokens_per_image + 1
    ids = torch.stack([torch.from_numpy(synth.make_prompt(cfg, L, image_positions=(35,), seed=60 + 97 * rank + i)) for i in range(B)])
    labels = ids.clone(); labels[:, :64] = -100; labels[ids == -200] = -100
    pix = torch.from_numpy(synth.make_pixels(cfg, B, seed=70 + rank)).to(dev, dtype)
    tower = model.get_vision_tower()

    def step():
        feats = tower(pix)                                         # frozen CLIP tower (clip_encoder.py:39-51), part of every step
        return ts.step(ids, labels, None, image_features=feats)

    losses = []
    # 288 GB per GPU: after one fully recomputing step (its peak is then known) the LAST layers' activations are kept up to what is left of 88 % of the device's
    # memory — every kept layer saves one forward of that layer per step (--train-keep-gb < 0: this rule, = 0: recompute everything, > 0: that many GB)
    torch.cuda.reset_peak_memory_stats(dev)
    losses.append(float(step()[0].item()))
    if a.train_keep_gb != 0:
        peak = torch.cuda.max_memory_allocated(dev)
        free_b, total_b = torch.cuda.mem_get_info(dev)
        other = max(0, total_b - free_b - torch.cuda.memory_reserved(dev))      # what is not torch's: the inference engine's weights (frozen tower) and workspaces
        ts.keep_budget_bytes = int(a.train_keep_gb * 1e9) if a.train_keep_gb > 0 else max(0, int(0.88 * total_b) - other - peak)
    for _ in range(max(1, a.warmup)):
        losses.append(float(step()[0].item()))
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        loss, count = step()
    barrier()
    dt = time.perf_counter() - t0
    losses.append(float(loss.item()))
    if a.dump_outputs and rank == 0:
        # before the phase split below, which steps the optimiser again: the loss, the label count and a fixed sample of the parameters the last step updated
        sample = torch.from_numpy(np.random.default_rng(0).choice(ts.flat_p.numel(), size=min(1 << 20, ts.flat_p.numel()), replace=False)).to(dev)
        dump_outputs(a.dump_outputs, {"loss": loss.reshape(1), "counted_labels": count.reshape(1), "params_sample": ts.flat_p[sample]})
    if world > 1:
        import torch.distributed as dist
        tt = torch.tensor([dt], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    # phase split (event-bracketed): forward only, forward + backward, optimiser
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    barrier()
    e[0].record(); ts.forward_backward(ids, labels, None, image_features=tower(pix), backward=False)
    e[1].record(); ts.forward_backward(ids, labels, None, image_features=tower(pix))
    e[2].record(); ts.optimizer_step()
    e[3].record(); torch.cuda.synchronize()
    n_param = ts.part.total
    tokens = B * T
    flops_step = 6.0 * (n_param - cfg.vocab_size * cfg.hidden_size) * tokens       # model FLOPs of the linears, forward + backward (the embedding lookup is no GEMM; recompute not counted)
    sys.stdout.flush()
    barrier()
    if rank == 0:
        line = {"metric": "training tokens/sec (visual-instruction-tuning step, LLaVA-1.5-7B, ZeRO-2 data parallel)", "value": world * tokens * a.steps / dt,
                "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": max(1, a.warmup), "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
                "config": {"workload": f"config5: {a.model} geometry, {B} x {T}-position samples per rank (1x336x336 image + {L}-token prompt each), LLM + mm_projector "
                                       f"trainable ({n_param / 1e9:.2f} B parameters), CLIP tower frozen, AdamW fp32 master + moments, max_grad_norm 1.0, activation recompute for "
                                       f"{ts.L - ts.last_kept_layers} of {ts.L} layers (the last {ts.last_kept_layers} keep their activations: --train-keep-gb), "
                                       f"ZeRO-2 over {world} rank(s) in {len(ts.part.buckets)} buckets", "parallelism": f"dp{world}",
                           "rccl_ranks": world if (world > 1 and not share) else 0},
                "forward_ms": e[0].elapsed_time(e[1]), "forward_backward_ms": e[1].elapsed_time(e[2]), "optimizer_ms": e[2].elapsed_time(e[3]),
                "linear_tflops_in_fwd_bwd": flops_step / (e[1].elapsed_time(e[2]) * 1e-3) / 1e12,
                "loss_first_last": [losses[0], losses[-1]], "grad_norm_last": ts.grad_norm(), "counted_labels": int(count.item()),
                "hbm_GB": {"params_grads": 2 * ts.flat_p.numel() * ts.flat_p.element_size() / 1e9, "optimizer_state": 3 * ts.master.numel() * 4 / 1e9,
                           "allocated_peak": torch.cuda.max_memory_allocated(dev) / 1e9,
                           "kept_activation_budget": (ts.keep_budget_bytes or 0) / 1e9, "kept_layers": ts.last_kept_layers,
                           "activation_bytes_per_layer": ts.layer_activation_bytes(_round_up_64(B * T)) / 1e9},
                "note": "attention backward on the matrix cores (csrc/attn_bwd.hip; LMX_ATTN_BWD_MFMA=0: the two-pass VALU kernels); wgrad from dy and x in their forward layout "
                        "(csrc/gemm8t.hip: LDS transpose reads, no transposed copies; bit-identical to the two-transpose path), dgrad = one weight transpose + the forward "
                        "GEMM; the forward's log-sum-exp kept for the backward; a layer's per-sample attention launches spread over --train-attn-streams side streams; layers whose activations fit the memory budget are not recomputed"}
        print(json.dumps(line), flush=True)
    barrier()


def _round_up_64(n):
    return (int(n) + 63) // 64 * 64


def run_config3(a, model, cfg, synth, dev, dtype, barrier, world, rank, share, build_s):
    """BASELINE config 3: LLaVA-1.5-13B geometry, batch = 8 images (8 requests, own image + own 512-token prompt each), chunked prefill (the rows of the
    8 requests walked as one packed block in pieces of 8 x 512 rows: lmx_prefill_batch), then the 8 sequences decode TOGETHER (one pass over the weights per step).  Tensor-parallel when launched with
    N > 1 ranks (config 3 proper is TP=2): every rank runs this same plan, so the engine calls match rank for rank."""
    from llava_mi355x import _C
    from llava_mi355x.batching import DecodeBatch
    from llava_mi355x.model import LmxKVCache
    B, chunk = 8, 512
    prompts = [torch.from_numpy(synth.make_prompt(cfg, a.prompt_len, image_positions=(35,), seed=20 + i))[None].to(dev) for i in range(B)]
    images = [torch.from_numpy(synth.make_pixels(cfg, 1, seed=40 + i)).to(dev, dtype) for i in range(B)]
    T = a.prompt_len - 1 + cfg.tokens_per_image

    def step():
        outs = model.generate_batch(prompts, images, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens, prefill_chunk=chunk, capacity=B)
        assert all(o.numel() == a.prompt_len + a.new_tokens for o in outs)
        return outs

    first = None
    for _ in range(max(1, a.warmup)):
        first = step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        last = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        tt = torch.tensor([dt], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    same = all(torch.equal(x, y) for x, y in zip(first, last))
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"output_ids": torch.stack([o.reshape(-1) for o in last])})
    # phase split: the 8 chunked prefills, then 127 batched decode steps (event-bracketed replay)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    barrier()
    e[0].record()
    caches, packed = [], []
    for ids, img in zip(prompts, images):
        _, _, _, _, embeds, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, img)
        caches.append(LmxKVCache(model, 1)); packed.append(embeds[0].contiguous())
    import ctypes as _ct
    arr = (_ct.c_void_p * B)(*[c.seqs[0].value if isinstance(c.seqs[0], _ct.c_void_p) else c.seqs[0] for c in caches])
    eptr = (_ct.c_void_p * B)(*[t.data_ptr() for t in packed]); cnt = (_ct.c_int32 * B)(*[int(t.shape[0]) for t in packed])
    _C.check(_C.lib.lmx_prefill_batch(model._h, arr, B, eptr, cnt, chunk * B, 1, _C.stream_handle()))      # the packed prefill generate_batch runs
    e[1].record()
    bt = DecodeBatch(model, B)
    bt.step([c.seqs[0] for c in caches], None, a.new_tokens - 1, True, want_ids=False)
    e[2].record()
    torch.cuda.synchronize()
    prefill_ms, decode_ms = e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
    bt.close()
    for c in caches:
        c.close()
    fl = flops_prefill(cfg, T, 1)
    try:
        import ctypes as _ct
        _ct.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    sys.stdout.flush()
    barrier()
    if rank == 0:
        line = {"metric": "generated tokens/sec + prefill ms (8 x [336px img + 512-tok prompt], chunked prefill), LLaVA-1.5-13B", "value": B * a.new_tokens * a.steps / dt,
                "unit": "generated tokens/s (whole job: 8 image encodes + 8 chunked prefills + 127 batched decode steps)", "n_gpus": world, "steps": a.steps,
                "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "strong" if world > 1 else "weak", "vs_baseline": None,
                "dtype": a.dtype, "data": "synthetic (seeded images + ids, random-init HF-std weights)",
                "config": {"workload": f"config3: {a.model}, batch 8 = 8 x (1x336x336 image + {a.prompt_len}-token prompt = {T} positions), packed prefill in pieces of {chunk * B} rows ({chunk} per request), "
                                       f"greedy {a.new_tokens} new tokens per request, the 8 sequences decode together", "parallelism": f"tp{world}", "kv_capacity": 2048,
                           "rccl_ranks": model.tp_comm_ranks() if world > 1 else None},
                "prefill_ms_8_requests": prefill_ms, "prefill_ms_per_request": prefill_ms / B,
                "prefill_frac_of_mfma_peak": B * fl["total"] / (prefill_ms * 1e-3) / 1e12 / (PEAK_BF16_TFLOPS * world),
                "decode_tokens_per_s": B * (a.new_tokens - 1) / (decode_ms * 1e-3), "decode_ms_per_step": decode_ms / (a.new_tokens - 1),
                "model_build_s": build_s, "greedy_ids_identical_across_steps": bool(same)}
        print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        if world == 1 and a.gpus > 1:
            raise SystemExit("--gpus N > 1 must be launched with torch.distributed.run --nproc-per-node N")
    # LMX_BENCH_SHARE_GPU=1 (dry run of the N>1 code path on a one-GPU box): every rank uses GPU 0, gloo instead of RCCL for
    # the host-side rendezvous and the engine's all-reduces all go through the P2P kernel (set LMX_TP_P2P_ALL=1 as well)
    share = os.environ.get("LMX_BENCH_SHARE_GPU") == "1"
    if share:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    if world > 1:
        import torch.distributed as dist
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)

    from synthetic import build as harness, recipes as synth
    if a.workload == "config3":
        a.model = "llava15_13b"
    cfg = synth.CONFIGS[a.model]
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    t0 = time.time()
    dp_only = a.workload == "config5"            # data parallel: every rank holds the whole (inference) model for its frozen tower
    model = harness.build_model(cfg, dtype=dtype, seed=0, device_rng=True, device=dev, tp_rank=0 if dp_only else rank, tp_world=1 if dp_only else world,
                                max_position=2048, gemm_variant=a.gemm_variant)
    if not dp_only:
        model.init_tensor_parallel(rccl=not share)
    build_s = time.time() - t0

    ids = torch.from_numpy(synth.make_prompt(cfg, a.prompt_len, image_positions=(35,), seed=2))[None].to(dev)
    pix = torch.from_numpy(synth.make_pixels(cfg, 1, seed=1)).to(dev, dtype)
    T = a.prompt_len - 1 + cfg.tokens_per_image
    torch.cuda.synchronize()

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier() if share else dist.barrier(device_ids=[local])
        torch.cuda.synchronize()

    if a.workload == "config3":
        run_config3(a, model, cfg, synth, dev, dtype, barrier, world, rank, share, build_s)
        return
    if a.workload == "config5":
        run_config5(a, model, cfg, synth, dev, dtype, barrier, world, rank, share, build_s)
        return

    def step():
        out = model.generate(inputs=ids, images=pix, do_sample=False, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens)
        assert out.shape[1] == a.prompt_len + a.new_tokens
        return out

    outs = []
    for _ in range(a.warmup):
        outs.append(step())
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        outs.append(step())
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        tt = torch.tensor([dt], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    deterministic = all(torch.equal(outs[0], o) for o in outs[1:])     # same request -> same greedy ids every step
    ms_per_step = dt / a.steps * 1e3
    value = a.new_tokens * a.steps / dt

    # ---- --full: phase split + per-kernel durations from profiled replays of the same step (HIP events on the launch stream) ----
    prefill_ms = decode_ms = roof = roof_p = breakdown = None
    if a.full:
        prefill_ms, decode_ms, roof, roof_p, breakdown = profile_request(a, model, cfg, dev, ids, pix, T, world, rank, barrier, step)

    # ---- N > 1: the weak-scaling job — N requests (one per GPU, own image + own prompt) as ONE tensor-parallel job: the tower data parallel over the
    #      images, packed prefill, the N sequences decoding together (model.generate_batch; every rank runs the same plan).  This is the workload the
    #      line's `value` is quoted on at N > 1 (DESIGN.md §4 "Multi-GPU"); the single request over TP = N stays beside it as `strong_single_request`
    weak, last_w = None, None
    if world > 1 and not a.no_weak:
        import torch.distributed as dist
        try:
            pw, iw = weak_job_inputs(cfg, dev, dtype, world, a.prompt_len)

            def step_w():
                o = model.generate_batch(pw, iw, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens, prefill_chunk=512, capacity=world)
                assert all(x.numel() == a.prompt_len + a.new_tokens for x in o)
                return o

            first_w = None
            for _ in range(max(1, min(a.warmup, 2))):
                first_w = step_w()
            barrier()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                last_w = step_w()
            barrier()
            dtw = time.perf_counter() - t0
            ttw = torch.tensor([dtw], device="cpu" if share else dev, dtype=torch.float64)
            dist.all_reduce(ttw, op=dist.ReduceOp.MAX)
            dtw = float(ttw.item())
            weak = {"what": f"{world} requests, one per GPU, as one TP = {world} job: image tower data parallel over the ranks + feature all-gather, packed prefill in pieces "
                            f"of {world} x 512 rows, {world} sequences decoding together", "requests": world, "scaling": "weak",
                    "value": world * a.new_tokens * a.steps / dtw, "ms_per_step": dtw / a.steps * 1e3,
                    "tower_sharded": bool(model.tower_is_sharded(world)),
                    "greedy_ids_identical_across_steps": bool(all(torch.equal(x, y) for x, y in zip(first_w, last_w)))}
        except Exception as ex:  # noqa: BLE001 — the line keeps the single-request measurement as its value and says why
            weak = {"error": repr(ex)}

    if a.dump_outputs and rank == 0:
        # the ids the caller of the timed path received in the last timed step: the weak job's N sequences when it is the headline, else the one request
        dump_outputs(a.dump_outputs, {"output_ids": torch.stack([x.reshape(-1) for x in last_w]) if weak and "value" in weak else outs[-1]})

    # ---- N > 1: the same N GPUs as N independent replicas (SURVEY §8e "data-parallel serving fallback": one full model per GPU, one
    #      request each, no collective) — reported next to the tensor-parallel `value`, never instead of it
    replicas = None
    one_gpu_same_job = None
    if a.full and world > 1 and not a.no_replicas:
        import torch.distributed as dist
        del outs
        full = harness.build_model(cfg, dtype=dtype, seed=0, device_rng=True, device=dev, tp_rank=0, tp_world=1, max_position=2048)
        ids_r = torch.from_numpy(synth.make_prompt(cfg, a.prompt_len, image_positions=(35,), seed=2 + rank))[None].to(dev)

        def step_r():
            return full.generate(inputs=ids_r, images=pix, do_sample=False, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens)

        for _ in range(max(1, a.warmup)):
            step_r()
        barrier()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step_r()
        barrier()
        dtr = time.perf_counter() - t0
        ttr = torch.tensor([dtr], device="cpu" if share else dev, dtype=torch.float64)
        dist.all_reduce(ttr, op=dist.ReduceOp.MAX)
        dtr = float(ttr.item())
        replicas = {"what": f"{world} independent full-model replicas, one request each, no collective", "scaling": "weak",
                    "value": world * a.new_tokens * a.steps / dtr, "ms_per_step": dtr / a.steps * 1e3}
        # the like-for-like yardstick of the weak job: the SAME world requests on ONE GPU (rank 0's full replica batches them: packed prefill + one decode
        # batch) while the other ranks idle — what tensor parallelism has to beat, measured in this run
        try:
            if rank == 0:
                pw1, iw1 = weak_job_inputs(cfg, dev, dtype, world, a.prompt_len)

                def step_1():
                    return full.generate_batch(pw1, iw1, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens, prefill_chunk=512, capacity=world)
                step_1()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step_1()
                torch.cuda.synchronize()
                dt1 = time.perf_counter() - t0
                one_gpu_same_job = {"what": f"the weak job's {world} requests batched on ONE GPU (TP = 1 full model: packed prefill + {world} sequences decoding together)",
                                    "value": world * a.new_tokens * a.steps / dt1, "ms_per_step": dt1 / a.steps * 1e3}
            barrier()
        except Exception as ex:  # noqa: BLE001
            one_gpu_same_job = {"error": repr(ex)}
            barrier()
        del full
        torch.cuda.empty_cache()

    # ---- serving-side view (BASELINE configs 3/4 run many requests at once): the same request x B decoding together through
    #      lmx_decode_batch (continuous batching) — aggregate generated tokens/s of the decode phase, not part of `value`
    serving = None
    if a.full and world == 1 and not a.no_batch:
        from llava_mi355x import _C
        from llava_mi355x.batching import DecodeBatch
        from llava_mi355x.model import LmxKVCache
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        serving = {"what": "decode phase of B identical config-2 requests stepping together (lmx_decode_batch), context %d" % T, "by_batch": {}}
        _, _, _, _, embeds, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, pix)
        sizes = [8, 16, 32]
        caches = []
        for _ in range(max(sizes)):
            c = LmxKVCache(model, 1)
            _C.check(_C.lib.lmx_prefill(model._h, c.seqs[0], _C.ptr(embeds[0]), embeds.shape[1], 0, None, 0, 1, _C.stream_handle()))
            caches.append(c)
        bt = DecodeBatch(model, max(sizes))
        for Bn in sizes:
            seqs = [c.seqs[0] for c in caches[:Bn]]
            bt.step(seqs, None, 2, True, want_ids=False)
            torch.cuda.synchronize()
            e[0].record(); bt.step(seqs, None, 16, True, want_ids=False); e[1].record()
            torch.cuda.synchronize()
            ms = e[0].elapsed_time(e[1]) / 16
            serving["by_batch"][str(Bn)] = {"ms_per_step": ms, "decode_tokens_per_s": Bn * 1e3 / ms}
        bt.close()
        for c in caches:
            c.close()

    # ---- live parity probe: the timed 16-bit kernels against the fp32 VERIFICATION engine (same orchestration, exact fp32 GEMM / attention; itself within
    # 1.5e-4 of the fp32 CPU oracle over all 1087 positions, tests/test_full_depth_gpu.py) on the SAME parameters (the seed's weights rounded to the 16-bit dtype), on
    # this build: last-position prefill logits and the first greedy ids of the timed request.  Not the oracle (minutes of host time) — a figure that moves with the kernels.
    live_parity = None
    if a.full and rank == 0 and world == 1 and not a.no_parity_probe:
        try:
            n_ids = 8
            lg16 = model.forward(input_ids=ids, images=pix, use_cache=False).logits[0, -1].float()
            ids16 = outs[-1][0, a.prompt_len:a.prompt_len + n_ids].tolist()
            m32 = harness.build_model(cfg, dtype=torch.float32, seed=0, device_rng=True, device=dev, max_position=2048, round_weights_to=dtype)
            lg32 = m32.forward(input_ids=ids, images=pix.float(), use_cache=False).logits[0, -1].float()
            g32 = m32.generate(inputs=ids, images=pix.float(), do_sample=False, max_new_tokens=n_ids, eos_token_id=-1)
            ids32 = g32[0, a.prompt_len:].tolist()
            scale = lg32.abs().max().item()
            noise = (lg16 - lg32).abs().max().item()
            live_parity = {"reference": "fp32 verification engine of this build on the same (16-bit-rounded) weights", "dtype": a.dtype,
                           "last_position_logits_max_abs_err": noise, "max_abs_logit": scale, "err_of_max_logit": noise / scale,
                           "rms_err_of_max_logit": (lg16 - lg32).pow(2).mean().sqrt().item() / scale, "argmax_equal": bool(lg16.argmax() == lg32.argmax()),
                           "greedy_ids_16bit": ids16, "greedy_ids_fp32": ids32,
                           # ids before the first difference (after it the two continuations are different sequences: nothing to compare position by position)
                           "greedy_ids_identical_prefix": next((i for i, (x, y) in enumerate(zip(ids16, ids32)) if x != y), n_ids), "greedy_ids_compared": n_ids}
            del m32, lg32, g32
            torch.cuda.empty_cache()
        except Exception as ex:  # noqa: BLE001
            live_parity = {"error": repr(ex)}

    tp_proj = None
    if a.full and rank == 0 and world == 1 and not a.no_tp_projection:
        try:
            tp_proj = tp_projection(cfg, dtype, dev, ids, pix, a.new_tokens)
            b32 = (serving or {}).get("by_batch", {}).get("32", {}).get("decode_tokens_per_s")
            # the weak-scaling jobs (W requests) on THIS one GPU, really run: what one GPU makes of the same W requests by batching alone
            one_gpu_jobs = {}
            for k in tp_proj["by_world"]:
                pw, iw = weak_job_inputs(cfg, dev, dtype, int(k), a.prompt_len)
                ts = []
                for r in range(3):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    model.generate_batch(pw, iw, max_new_tokens=a.new_tokens, eos_token_id=-1, run_ahead=a.new_tokens, prefill_chunk=512, capacity=int(k))
                    torch.cuda.synchronize()
                    if r:
                        ts.append(time.perf_counter() - t0)
                one_gpu_jobs[k] = {"job_ms": min(ts) * 1e3, "value_tokens_per_s": int(k) * a.new_tokens / min(ts)}
            tp_proj["measured_tp1"] = {"prefill_ms": prefill_ms, "decode_ms_per_token": decode_ms / (a.new_tokens - 1), "value": value, "batch32_decode_tokens_per_s": b32,
                                       "same_jobs_on_one_gpu": one_gpu_jobs}
            for k, v in tp_proj["by_world"].items():
                v["projected_speedup_vs_tp1"] = v["projected_value_tokens_per_s"] / value
                if b32:
                    v["projected_batch32_speedup_vs_tp1"] = v["p2p"]["projected_batch_decode_tokens_per_s"] / b32
                wk = v.get("weak")
                if wk:
                    wk["projected_speedup_vs_one_gpu_one_request"] = wk["projected_value_tokens_per_s"] / value            # the driver's scaling ratio: value(N) / value(1)
                    wk["projected_vs_replicas"] = wk["projected_value_tokens_per_s"] / (int(k) * value)                     # > 1: one TP group beats N independent GPUs
                    wk["projected_vs_same_job_on_one_gpu"] = wk["projected_value_tokens_per_s"] / one_gpu_jobs[k]["value_tokens_per_s"]
        except Exception as ex:  # noqa: BLE001
            tp_proj = {"error": repr(ex)}

    cpu = None
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        try:
            need_gb = sum(int(torch.tensor(shp).prod()) for shp in synth.tensor_shapes(cfg).values()) * 2 / 1e9 + 16
            avail_gb = next((int(l.split()[1]) / 1e6 for l in open("/proc/meminfo") if l.startswith("MemAvailable")), 0.0)
            if a.cpu_layers > 0 or avail_gb < need_gb:
                cpu = cpu_baseline(cfg, T, a.new_tokens, a.cpu_layers or 2)
            else:
                del outs
                torch.cuda.empty_cache()
                ref = None
                if not a.no_cpu_reference:
                    try:
                        ref = cpu_baseline_reference(cfg, ids, pix.float(), a.new_tokens, a.cpu_decode_steps)
                    except Exception as ex:  # noqa: BLE001 — version skew of the host stack must not cost the line its baseline
                        ref = {"error": repr(ex)}
                # the oracle restatement ("port"): the whole request when it is the only baseline, a shorter sample beside the reference's own code
                have_ref = bool(ref) and "value" in ref
                port = cpu_baseline_full(cfg, ids, pix.float(), a.new_tokens, not a.no_cpu_fp32, a.cpu_decode_steps or (16 if have_ref else 0), prefill_runs=1 if have_ref else 3)
                if have_ref:
                    cpu = ref
                    cpu["port"] = port
                    cpu["port_vs_reference"] = port["value"] / ref["value"]
                else:
                    cpu = port
                    if ref:
                        cpu["reference_error"] = ref.get("error")
        except Exception as ex:  # noqa: BLE001
            cpu = {"error": repr(ex)}

    # Native libraries write to C stdio (RCCL prints a version banner on its first communicator), which is block-buffered on a pipe and
    # would otherwise come out at process exit, AFTER the JSON line.  Every rank flushes it now, then rank 0 prints the JSON line last.
    try:
        import ctypes as _ct
        _ct.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    sys.stdout.flush()
    barrier()
    if rank == 0:
        # the tensor-parallel PROJECTION (rank-local shards timed on this one GPU + a link model: a model, not a measurement) goes to a side file; the line keeps
        # its headline ratios and says where the rest is
        tp_brief = None
        if tp_proj is not None:
            tp_brief = {"what": "PROJECTION, unmeasured on hardware: rank-local shards of TP 2 / 4 / 8 timed on this GPU with a no-op all-reduce + a link model",
                        "error": tp_proj.get("error")}
            try:
                side = os.path.join(ROOT, "gpurun_out", "bench_tp_projection.json")
                os.makedirs(os.path.dirname(side), exist_ok=True)
                with open(side, "w") as f:
                    json.dump(tp_proj, f, indent=1)
                tp_brief["file"] = os.path.relpath(side, ROOT)
                w8 = (tp_proj.get("by_world") or {}).get("8") or {}
                tp_brief["tp8"] = {"single_request_speedup_vs_tp1": w8.get("projected_speedup_vs_tp1"),
                                   "weak_job_vs_eight_replicas": (w8.get("weak") or {}).get("projected_vs_replicas"),
                                   "weak_job_vs_same_job_on_one_gpu": (w8.get("weak") or {}).get("projected_vs_same_job_on_one_gpu"),
                                   "batch32_decode_speedup_vs_tp1": w8.get("projected_batch32_speedup_vs_tp1")}
            except Exception as ex:  # noqa: BLE001
                tp_brief["error"] = repr(ex)
        strong = None
        decode_tok_ms = decode_ms / (a.new_tokens - 1) if a.full else None
        workload = f"{a.model}: 1x336x336 image + {a.prompt_len}-token prompt ({T} positions), greedy {a.new_tokens} new tokens, batch 1"
        scaling = "strong" if world > 1 else "weak"
        if weak and "value" in weak:
            # N > 1: `value` is the weak-scaling job (per-GPU work fixed: one request per GPU); the single request over TP = N is reported beside it
            strong = {"what": f"ONE request over TP = {world} (latency view; total work fixed)", "scaling": "strong", "value": value, "ms_per_step": ms_per_step,
                      "prefill_ms": prefill_ms, "decode_ms_per_token": decode_tok_ms, "greedy_ids_identical_across_steps": bool(deterministic)}
            value, ms_per_step, scaling = weak["value"], weak["ms_per_step"], "weak"
            workload = (f"{a.model}: {world} requests (one per GPU), each 1x336x336 image + {a.prompt_len}-token prompt ({T} positions), greedy {a.new_tokens} new tokens; "
                        f"one TP = {world} job (tower data parallel, packed prefill, {world} sequences decoding together)")
        line = {"metric": "generated tokens/sec + prefill ms (336px img + 512-tok prompt), LLaVA-1.5-7B", "value": value,
                "unit": "generated tokens/s (whole request: image encode + prefill + decode)" if scaling != "weak" or world == 1 else
                        "generated tokens/s (whole job: image encodes + packed prefill + batched decode of one request per GPU)",
                "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "full": a.full,
                "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
                "dtype": a.dtype, "data": "synthetic (seeded image + ids, random-init HF-std weights)",
                "config": {"workload": workload,
                           "parallelism": f"tp{world}", "kv_capacity": 2048,
                           "decode_allreduce": ("p2p-one-shot" if getattr(model, "p2p_active", False) else "rccl") if world > 1 else None,
                           "rccl_ranks": model.tp_comm_ranks() if world > 1 else None, "prefill_allreduce": ("rccl on the engine's comm stream, two row halves overlapped with the other half's GEMMs"
                                                 if T * world >= 4096 else "rccl on the launch stream (the two-half pipeline starts at rows x ranks >= 4096)") if world > 1 else None},
                # null without --full: the phase split, the rooflines, cpu_baseline, serving_batch, replicas, tp_projection, parity, same_job_on_one_gpu*, kernel_breakdown
                "prefill_ms": prefill_ms, "decode_tokens_per_s": 1e3 / decode_tok_ms if a.full else None, "decode_ms_per_token": decode_tok_ms,
                # the two whole-phase fractions at the top level: every algorithmic byte of a decode step over the wall time per token against
                # the HBM peak, and every FLOP of the prefill (tower + projector + decoder) over the measured prefill time against the dense bf16 MFMA peak
                "decode_step_frac_of_hbm_peak": ((roof or {}).get("decode_step") or {}).get("frac"), "prefill_frac_of_mfma_peak": (roof_p or {}).get("frac"),
                "roofline": roof, "roofline_prefill": roof_p, "cpu_baseline": cpu, "serving_batch": serving, "weak_job": weak, "strong_single_request": strong,
                "replicas": replicas, "tp_projection": tp_brief,
                # N > 1 — what `value` is and the two numbers it must be read against, at the top level (VERDICT r4 weak 10 / ADVICE r4): `value` = the WEAK job
                # (N requests as one TP = N job); it is NOT an N-fold tensor-parallel speed-up of one request
                "schema": 6, "parity": dict(parity_record(a.model), live=live_parity) if a.full else None,
                "value_definition": ("one request (N = 1)" if world == 1 else f"weak-scaling job: {world} requests, one per GPU, run as ONE TP = {world} job; compare with "
                                     "strong_single_request_value (ONE request over the same GPUs) and same_job_on_one_gpu_value (the same requests batched on one GPU)"),
                "strong_single_request_value": (strong or {}).get("value") if world > 1 else None,
                "same_job_on_one_gpu_value": (one_gpu_same_job or {}).get("value") if world > 1 else None,
                "value_vs_same_job_on_one_gpu": (value / one_gpu_same_job["value"]) if world > 1 and one_gpu_same_job and "value" in one_gpu_same_job else None,
                "same_job_on_one_gpu": one_gpu_same_job,
                "kernel_breakdown_ms_per_step": breakdown,
                "model_build_s": build_s, "greedy_ids_identical_across_steps": bool(deterministic)}
        print(json.dumps(line), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def profile_request(a, model, cfg, dev, ids, pix, T, world, rank, barrier, step):
    """--full: phase split (prefill / decode) and in-situ per-kernel durations of profiled replays of the timed request, priced against the rooflines."""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    from llava_mi355x.model import LmxKVCache
    from llava_mi355x import _C
    prefill_ms, decode_ms = [], []
    for _ in range(max(2, a.steps)):
        barrier()
        e[0].record()
        _, _, _, _, embeds, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, pix)
        cache = LmxKVCache(model, 1)
        _C.check(_C.lib.lmx_prefill(model._h, cache.seqs[0], _C.ptr(embeds[0]), embeds.shape[1], 0, None, 0, 1, _C.stream_handle()))
        e[1].record()
        _C.check(_C.lib.lmx_decode(model._h, cache.seqs[0], -1, a.new_tokens - 1, None, 1, _C.stream_handle()))
        e[2].record()
        torch.cuda.synchronize()
        prefill_ms.append(e[0].elapsed_time(e[1])); decode_ms.append(e[1].elapsed_time(e[2]))
        cache.close()
    prefill_ms = sorted(prefill_ms)[len(prefill_ms) // 2]
    decode_ms = sorted(decode_ms)[len(decode_ms) // 2]

    # in-situ per-kernel profile: three profiled requests, per scope the MEDIAN of the three totals — a single pass put one stray o_proj launch (a 0.9 ms hiccup among 32
    # launches of 55 us) into a committed line as "o_proj 432 TF/s"
    profs = []
    for _ in range(3):
        model.profile(True)
        step()
        profs.append(model.profile_read())
        model.profile(False)
    prof = {}
    for k in profs[0]:
        have = sorted((p[k] for p in profs if k in p), key=lambda v: v[0])
        prof[k] = have[len(have) // 2]

    fl = flops_prefill(cfg, T, 1)
    H, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.vocab_size
    # decode GEMV family: algorithmic bytes = weight bytes streamed per launch (13.214 GB / token for 7B)
    es = 2
    # split-q decode step (csrc/decode_attn.hip): the q|k|v projection runs as a q launch (a plain gemv2_kernel launch: in the family) + ONE launch that streams the
    # k | v weight rows AND the layer's K / V^T cache with the attention's latency chain inside (decode_kv_attn_kernel: reported beside the family, roofline.kv_attn)
    kv_launch = 2.0 * (T + a.new_tokens / 2.0) * cfg.num_key_value_heads * cfg.head_dim * es / world        # KV bytes per layer at the mean context of the timed steps
    gemv_bytes = {"decode.gemv.qkv": 3 * H * H * es / world, "decode.gemv.q": H * H * es / world,
                  "decode.gemv.o": H * H * es / world, "decode.gemv.gate_up": 2 * H * I * es / world,
                  "decode.gemv.down": H * I * es / world, "decode.gemv.lm_head": V * H * es}
    gb = sum(gemv_bytes[k] * prof[k][1] for k in gemv_bytes if k in prof)
    gs = sum(prof[k][0] for k in gemv_bytes if k in prof) * 1e-3
    n_gemv = sum(prof[k][1] for k in gemv_bytes if k in prof)
    # every per-launch figure of the in-situ profile carries the cost of its HIP event pair; calibrate_event_overhead measures it around a
    # real kernel (at TP=1 the all-reduce scope brackets nothing and shows the larger empty-scope latency, reported next to it)
    empty_scope_us = prof["decode.allreduce"][0] / max(prof["decode.allreduce"][1], 1) * 1e3 if world == 1 and "decode.allreduce" in prof else None
    marker_us, cal_t1, cal_t2 = calibrate_event_overhead(dev)
    # HBM-side traffic per launch: measured in THIS run by two rocprofv3 --pmc passes over the cold-cache single-kernel driver
    # (pmc_traffic); falls back to the committed passes of profiles/ when rocprofv3 is unavailable
    traffic, traffic_src = None, None
    if rank == 0 and world == 1 and a.model == "llava15_7b" and not a.no_pmc:
        pm = pmc_traffic(ROOT)
        if pm and "ratio" in pm:
            traffic, traffic_src = pm["ratio"] * gb / max(n_gemv, 1), {"how": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, this run (tools/mb_gemv_cold.py)", **pm}
        elif pm:
            traffic_src = pm
    if traffic is None and world == 1 and a.model == "llava15_7b":
        try:
            with open(os.path.join(ROOT, "profiles", "r01_pmc_traffic.json")) as f:
                pt = json.load(f)["gemv_kernel"]
            ratio = sum(v["hbm_bytes"] for v in pt.values()) / sum(v["algorithmic_bytes"] for v in pt.values())
            traffic = ratio * gb / max(n_gemv, 1)
            traffic_src = {"how": "committed passes profiles/r01_pmc_traffic.json (no live PMC in this run)", "ratio": ratio, "live_error": traffic_src}
        except Exception:  # noqa: BLE001
            traffic = None
    # GEMV / GEMM scopes are timed by the launch's own start / stop events (hipExtLaunchKernelGGL): kernel-only durations, directly comparable with the
    # rocprofv3 kernel stats of the same command (profiles/r02_rocprofv3_kernel_stats_final.csv).  Every other entry of kernel_breakdown still carries
    # the cost of a stream-marker pair (event_pair_overhead_us)
    gs_k = gs
    roof = {"bound": "hbm", "kernel": "gemv2_body<bf16,R,P> (csrc/gemv2.h: hand-counted weight stream) as gemv2_kernel launches: q, o_proj, gate|up, down, lm_head of a decode step incl. fused RMSNorm / SiLU·mul / residual; the k | v rows run inside decode_kv_attn_kernel, see kv_attn",
            "achieved": gb / max(gs_k, 1e-12) / 1e9, "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": gb / max(gs_k, 1e-12) / 1e9 / PEAK_HBM_GBS,
            "launches": int(n_gemv), "avg_launch_us": gs_k / max(n_gemv, 1) * 1e6, "bytes_per_token": (H * H * es * L / world if "decode.kv_attn" in prof else 3 * H * H * es * L / world) + H * H * es * L / world + 3 * H * I * es * L / world + V * H * es,
            "traffic": traffic, "traffic_source": traffic_src, "traffic_unit": "HBM-side bytes per launch; algorithmic = %.0f" % (gb / max(n_gemv, 1)),
            "measured": "start / stop events of hipExtLaunchKernelGGL on every GEMV launch (stamped at the kernel's own begin and end on its stream: kernel-only "
                        "durations, what rocprofv3 --kernel-trace reports) in a profiled replay of the timed step, same process"}
    if "decode.kv_attn" in prof and prof["decode.kv_attn"][1] > 0:
        kb = 2 * H * H * es / world + kv_launch
        kt_ = prof["decode.kv_attn"][0] * 1e-3 / prof["decode.kv_attn"][1]
        roof["kv_attn"] = {"kernel": "decode_kv_attn_kernel (k | v projection rows through gemv2_body + the layer's attention workgroups; the launch ends ~2 us after the projection: "
                                     "hand-over of the newest key / value to the heads' mergers)", "algorithmic_bytes": kb, "weights_bytes": 2 * H * H * es / world, "kv_cache_bytes": kv_launch,
                           "avg_launch_us": kt_ * 1e6, "launches": int(prof["decode.kv_attn"][1]), "achieved": kb / kt_ / 1e9, "frac": kb / kt_ / 1e9 / PEAK_HBM_GBS, "unit": "GB/s"}
    # the whole decode step against the HBM peak: every algorithmic byte of a token (weights + KV at the mean context) over the measured time per token
    step_bytes = 4 * H * H * es * L / world + 3 * H * I * es * L / world + V * H * es + kv_launch * L
    roof["decode_step"] = {"bytes_per_token": step_bytes, "ms_per_token": decode_ms / (a.new_tokens - 1), "achieved": step_bytes / (decode_ms / (a.new_tokens - 1) * 1e-3) / 1e9,
                           "frac": step_bytes / (decode_ms / (a.new_tokens - 1) * 1e-3) / 1e9 / PEAK_HBM_GBS, "unit": "GB/s",
                           "what": "weights + K / V^T cache of one token / wall time per token (launch boundaries, attention chain and pick included)"}
    gemm_flops = {"prefill.gemm.qkv": 2.0 * T * 3 * H * H / world, "prefill.gemm.o": 2.0 * T * H * H / world,
                  "prefill.gemm.gate_up": 2.0 * T * 2 * H * I / world, "prefill.gemm.down": 2.0 * T * H * I / world}
    gf = sum(gemm_flops[k] * prof[k][1] for k in gemm_flops if k in prof)
    gt = sum(prof[k][0] for k in gemm_flops if k in prof) * 1e-3
    n_gemm = sum(prof[k][1] for k in gemm_flops if k in prof)
    gt_k = gt
    mfma_busy, pmc_file = None, None
    for cand in ("r06_pmc.json", "r05_pmc.json", "r04_pmc.json", "r03_pmc.json", "r02_pmc_gemm.json"):
        try:
            with open(os.path.join(ROOT, "profiles", cand)) as f:
                mfma_busy = json.load(f).get("summary")
            pmc_file = cand
            break
        except Exception:  # noqa: BLE001
            continue
    # HBM-side bytes per GEMM launch: PMC passes (FETCH_SIZE + WRITE_SIZE with the guide's gfx950 corrections) over the single-kernel drivers, committed digest
    gemm_traffic = None
    live_gemm = None
    if rank == 0 and world == 1 and a.model == "llava15_7b" and not a.no_pmc:
        live_gemm = pmc_prefill_traffic(ROOT, T)
    if world == 1 and a.model == "llava15_7b" and live_gemm and "error" not in live_gemm:
        algo = {"qkv": (T * H + 3 * H * H + T * 3 * H) * es, "o_proj": (T * H + H * H + 2 * T * H) * es, "gate_up": (T * H + 2 * H * I + T * I) * es,
                "down": (T * I + H * I + 2 * T * H) * es}
        per = {k: {"hbm_side_bytes": live_gemm[k], "algorithmic_bytes": algo[k], "ratio": live_gemm[k] / algo[k]} for k in algo}
        gemm_traffic = {"per_launch_avg_bytes": sum(v["hbm_side_bytes"] for v in per.values()) / len(per), "by_shape": per,
                        "how": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, THIS run (tools/mb_gemm_prefill.py: the four shapes as the engine launches them); counted at the L2 -> fabric "
                               "boundary, so Infinity-Cache hits are inside; o_proj / down_proj are K-sliced (3 slices): their figure includes the fp32 partial tiles written by the "
                               "GEMM and read by the launch-boundary reduction; the rest above 1.0 is operand-tile re-reads that drift out of an XCD's 4 MB L2"}
    elif mfma_busy and world == 1 and a.model == "llava15_7b":
        algo = {"qkv": (T * H + 3 * H * H + T * 3 * H) * es, "o_proj": (T * H + H * H + 2 * T * H) * es, "gate_up": (T * H + 2 * H * I + T * I) * es,
                "down": (T * I + H * I + 2 * T * H) * es}
        per = {k: {"hbm_side_bytes": mfma_busy[k]["hbm_side_bytes"], "algorithmic_bytes": algo[k], "ratio": mfma_busy[k]["hbm_side_bytes"] / algo[k]}
               for k in algo if k in mfma_busy and "hbm_side_bytes" in mfma_busy[k]}
        if per:
            gemm_traffic = {"per_launch_avg_bytes": sum(v["hbm_side_bytes"] for v in per.values()) / len(per), "by_shape": per,
                            "live_error": live_gemm,
                            "how": f"profiles/{pmc_file} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/gpu_pmc_r3.sh over the single-shape drivers; committed digest, not "
                                   "re-measured in this run); counted at the L2 -> fabric boundary, so Infinity-Cache hits are inside; o_proj / down_proj are K-sliced (3 slices): "
                                   "their figure includes the fp32 partial tiles written by the GEMM and read by the launch-boundary reduction; the rest above 1.0 is operand-tile "
                                   "re-reads (each X tile by every N-tile column, each W tile by the 5 M-tiles) that drift out of an XCD's 4 MB L2"}
    roof_p = {"bound": "mfma", "kernel": "gemm8p_kernel<bf16,...> (q|k|v, gate|up whole tiles; o_proj, down_proj as 3 K slices + splitk_reduce_kernel, timed together): decoder prefill linears",
              # frac = the north_star quantity: ALL FLOPs of the prefill (tower + projector + decoder linears + attention) / the measured prefill time;
              # the GEMM family alone (kernel-only durations) is reported beside it
              "achieved": fl["total"] / (prefill_ms * 1e-3) / 1e12 / world, "peak": PEAK_BF16_TFLOPS,
              "unit": "TFLOP/s", "frac": fl["total"] / (prefill_ms * 1e-3) / 1e12 / (PEAK_BF16_TFLOPS * world), "frac_is": "prefill end to end (image encode + splice + decoder prefill), per GPU",
              "gemm_family_tflops": gf / gt_k / 1e12, "gemm_family_frac": gf / gt_k / 1e12 / PEAK_BF16_TFLOPS,
              "launches": int(n_gemm), "avg_launch_us": gt_k / max(n_gemm, 1) * 1e6,
              "by_shape_tflops": {k: gemm_flops[k] * prof[k][1] / max(prof[k][0] * 1e-3, 1e-9) / 1e12 for k in gemm_flops if k in prof},
              "traffic": gemm_traffic, "mfma_busy": mfma_busy, "prefill_total_tflop": fl["total"] / 1e12,
              "prefill_end_to_end_frac": fl["total"] / (prefill_ms * 1e-3) / 1e12 / (PEAK_BF16_TFLOPS * world),
              "measured": "start / stop events of hipExtLaunchKernelGGL on every GEMM launch (kernel-only durations) in a profiled replay of the timed step"}
    breakdown = {k: {"ms": round(v[0], 4), "n": int(v[1])} for k, v in sorted(prof.items())}
    roof["event_pair_overhead_us"] = marker_us
    roof["event_pair_calibration"] = {"one_launch_scope_us": cal_t1, "two_launch_scope_us": cal_t2, "empty_scope_us": empty_scope_us}
    roof_p["event_pair_overhead_us"] = marker_us
    return prefill_ms, decode_ms, roof, roof_p, breakdown


if __name__ == "__main__":
    main()
