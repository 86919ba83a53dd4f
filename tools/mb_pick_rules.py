"""Time the ruled pick (lmx_op_pick_rules: repetition penalty + no-repeat trigram over a 2048-id history) against the plain pick (lmx_op_argmax,
lmx_op_sample) at V = 32000, bf16 logits, greedy and top-p.  Back-to-back launches between two events; the phases alternate kernel names
(argmax, ruled greedy, sample, ruled top-p), so a kernel trace of this run splits into the four by order."""
import ctypes, json, os, random, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))
from llava_mi355x import _C
dev = torch.device("cuda:0")
V, N_HIST, N_OUT = 32000, 2048, 1024
logits = (torch.randn(V, device=dev) * 3).bfloat16()
rng = random.Random(3)
alphabet = rng.sample(range(V), 600)                    # a 2048-id text holds a few hundred distinct ids
hist = torch.tensor([rng.choice(alphabet) for _ in range(N_HIST)], dtype=torch.long, device=dev)
out = torch.zeros(1, dtype=torch.long, device=dev)
off = torch.zeros(1, dtype=torch.int32, device=dev)
none64 = (ctypes.c_int64 * 1)(0)
def t(fn, reps=200):
    for _ in range(10): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3
def ruled(T, p, k, penalty=1.3, ngram=3):
    return lambda: _C.check(_C.lib.lmx_op_pick_rules(_C.DTYPE_BF16, _C.ptr(logits), V, V, _C.ptr(hist), N_HIST, N_OUT, penalty, ngram, 0, none64, 0, none64, 0,
                                                     T, p, k, 7, None, _C.ptr(out), None, None, _C.stream_handle()))
res = {}
res["plain_greedy"] = t(lambda: _C.check(_C.lib.lmx_op_argmax(_C.DTYPE_BF16, _C.ptr(logits), V, _C.ptr(out), _C.stream_handle())))
res["ruled_greedy"] = t(ruled(0.0, 1.0, 0))
res["plain_T0.7_p0.9"] = t(lambda: _C.check(_C.lib.lmx_op_sample(_C.DTYPE_BF16, _C.ptr(logits), V, 0.7, 0.9, 0, 7, _C.ptr(off), None, _C.ptr(out), None, _C.stream_handle())))
res["ruled_T0.7_p0.9"] = t(ruled(0.7, 0.9, 0))
print(json.dumps({k: round(v, 2) for k, v in res.items()}))
