"""Cold-cache sweep of the rotated decode copies (csrc/gemv2.h ROT form): per 7B decode linear, the plain launch against rotation steps 1 / 3 / 5 / 7.

Like tools/mb_gemv_cold.py every arm cycles over distinct weight matrices per shape (no L2 / Infinity-Cache reuse, as in a real decode step); the arms of a
linear alternate inside every repeat, so drift hits all of them alike.  One JSON line per (linear, step) with the per-launch time of every repeat, and one
"verdict" line per linear: a step is kept only if its median beats the plain median by more than the spread (max - min) of the plain arm's repeats.

    python tools/mb_gemv_rot.py [--out profiles/gemv_rot_sweep.jsonl] [--repeats 7] [--copies 32]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))
from llava_mi355x import _C, ops  # noqa: E402

STEPS = (1, 3, 5, 7)
# name, N, K, fused RMSNorm, residual, activation — the launches of Model::decode_step_launch at LLaVA-1.5-7B ("kv": the k | v rows as a launch of their own)
LINEARS = [("down", 4096, 11008, False, True, _C.ACT_NONE), ("lm_head", 32000, 4096, True, False, _C.ACT_NONE), ("kv", 8192, 4096, True, False, _C.ACT_NONE),
           ("q", 4096, 4096, True, False, _C.ACT_NONE), ("o", 4096, 4096, False, True, _C.ACT_NONE), ("gate_up", 22016, 4096, True, False, _C.ACT_SILU_MUL)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--copies", type=int, default=32)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(o):
        lines.append(o)
        print(json.dumps(o), flush=True)

    for name, N, K, norm, resid, act in LINEARS:
        if a.only and name not in a.only.split(","):
            continue
        L = max(4, min(a.copies, (6 << 30) // (N * K * 2)))           # at least 6 GB or `copies` matrices per arm: far beyond the 256 MB memory-side cache
        torch.manual_seed(N + K)
        ws = [(torch.randn(N, K, device=dev) / math.sqrt(K)).bfloat16() for _ in range(L)]
        x = torch.randn(1, K, device=dev).bfloat16()
        g = torch.ones(K, device=dev).bfloat16() if norm else None
        n_out = N // 2 if act == _C.ACT_SILU_MUL else N
        r = torch.randn(1, n_out, device=dev).bfloat16() if resid else None
        out = torch.empty(1, n_out, device=dev, dtype=torch.bfloat16)
        ref = ops.gemv(x, ws[0], norm_w=g, residual=r, act=act).clone()
        arms = {0: ws}
        for s in STEPS:
            arms[s] = [ops.gemv_rot_pack(w, s, norm=norm, act=act) for w in ws]
            assert torch.equal(ops.gemv_rot(x, arms[s][0], K, s, norm_w=g, residual=r, act=act), ref), (name, s)

        def run(s):
            if s == 0:
                for w in arms[0]:
                    ops.gemv(x, w, norm_w=g, residual=r, act=act, out=out)
            else:
                for w in arms[s]:
                    ops.gemv_rot(x, w, K, s, norm_w=g, residual=r, act=act, out=out)

        times = {s: [] for s in arms}
        for s in arms:
            run(s)
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for s in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    run(s)
                e1.record()
                torch.cuda.synchronize()
                times[s].append(e0.elapsed_time(e1) / (5 * L) * 1e3)
        med = {s: sorted(t)[len(t) // 2] for s, t in times.items()}
        spread = max(times[0]) - min(times[0])
        for s, t in times.items():
            emit({"kind": "gemv_rot_sweep", "linear": name, "N": N, "K": K, "step": s, "copies": L, "us_median": round(med[s], 3), "us_min": round(min(t), 3),
                  "us_max": round(max(t), 3), "us": [round(v, 3) for v in t], "gbps": round(N * K * 2 / med[s] / 1e3, 1)})
        best = min(STEPS, key=lambda s: med[s])
        emit({"kind": "gemv_rot_verdict", "linear": name, "plain_us": round(med[0], 3), "plain_spread_us": round(spread, 3), "best_step": best,
              "best_us": round(med[best], 3), "gain_us": round(med[0] - med[best], 3), "keep": bool(med[0] - med[best] > spread)})
        del ws, arms
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for o in lines:
                f.write(json.dumps(o) + "\n")


if __name__ == "__main__":
    main()
