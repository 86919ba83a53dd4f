"""What asking generate() for scores costs at the benchmark geometry (bench.py's config2: LLaVA-1.5-7B synthetic weights, bf16, 336 px image + 512-token prompt,
128 new tokens, run_ahead = 128): the same request without the arguments, with return_dict_in_generate=True alone (log-probabilities only) and with
output_scores=True as well (full fp32 rows), greedy and sampled (T 0.7, top-p 0.9).  Whole requests between two synchronisations, the variants interleaved
round by round; prints one JSON line with ms per generated token (median over the rounds) and the difference to the plain request."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "llava-plus-codebase_amd"), ROOT):
    sys.path.insert(0, p)
from synthetic import build as harness, recipes as synth  # noqa: E402

NEW, PROMPT, ROUNDS, WARMUP = 128, 512, 7, 2
dev = torch.device("cuda:0")
cfg = synth.CONFIGS["llava15_7b"]
model = harness.build_model(cfg, dtype=torch.bfloat16, seed=0, device_rng=True, device=dev, max_position=2048)
ids = torch.from_numpy(synth.make_prompt(cfg, PROMPT, image_positions=(35,), seed=2))[None].to(dev)
pix = torch.from_numpy(synth.make_pixels(cfg, 1, seed=1)).to(dev, torch.bfloat16)
MODES = {"greedy": dict(do_sample=False), "sampled": dict(do_sample=True, temperature=0.7, top_p=0.9)}
ASKS = {"plain": {}, "logprobs": dict(return_dict_in_generate=True), "rows": dict(return_dict_in_generate=True, output_scores=True)}


def request(mode, ask):
    torch.manual_seed(11)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(inputs=ids, images=pix, max_new_tokens=NEW, eos_token_id=-1, run_ahead=NEW, **MODES[mode], **ASKS[ask])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    seq = out if isinstance(out, torch.Tensor) else out.sequences
    assert seq.shape[1] == PROMPT + NEW
    return dt, seq


times = {(m, a): [] for m in MODES for a in ASKS}
same_ids = True
for r in range(WARMUP + ROUNDS):
    for m in MODES:
        ref = None
        for a in ASKS:
            dt, seq = request(m, a)
            ref = seq if ref is None else ref
            same_ids = same_ids and torch.equal(seq, ref)
            if r >= WARMUP:
                times[(m, a)].append(dt)
res = {"device": torch.cuda.get_device_name(0), "new_tokens": NEW, "rounds": ROUNDS, "ids_equal_with_and_without_scores": bool(same_ids)}
for m in MODES:
    base = statistics.median(times[(m, "plain")]) / NEW * 1e3
    res[m] = {"plain_ms_per_token": round(base, 4)}
    for a in ("logprobs", "rows"):
        v = statistics.median(times[(m, a)]) / NEW * 1e3
        res[m][a + "_ms_per_token"] = round(v, 4)
        res[m][a + "_extra_ms_per_token"] = round(v - base, 4)
    res[m]["spread_plain_ms_per_token"] = round((max(times[(m, "plain")]) - min(times[(m, "plain")])) / NEW * 1e3, 4)
print(json.dumps(res))
