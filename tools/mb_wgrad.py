"""Weight-gradient GEMM at the 7B training shapes (16 x 2048 = 32768 rows): lmx_op_gemm_wgrad (csrc/gemm8t.hip, operands in their forward layout) against the path it
replaces (two lmx_op_transpose + lmx_op_gemm), and its accumulating form lmx_op_gemm_wgrad_acc (gradient accumulation: the prior gradient is read in the epilogue)
against the plain launch plus one read of the output.

Usage: python tools/mb_wgrad.py [rows] [--parent-lib PATH] [--jsonl PATH]
  --parent-lib   libllava_mi355x.so of the parent commit, built in a second checkout: its lmx_op_gemm_wgrad is timed in the same process, alternating with this
                 tree's, and the spread of its five repeats is the margin of both comparisons
  --jsonl        also append one JSON line per shape to this file (profiles/grad_accum_wgrad.jsonl holds a recorded run)
Per shape, five repeats of every variant (interleaved; each repeat times 5 launches between device events).  `*_us` are medians, `*_spread_us` max - min.
  plain_ok   plain_us <= parent_us + parent_spread_us                                  (needs --parent-lib)
  acc_ok     acc_us <= plain_us + read_us + margin, read_us = the time to read out x in 16-bit elements once at the rate a plain device copy of that size reaches
             in this run (copy_GBs counts its read and its write), margin = parent_spread_us (plain_spread_us without a parent): the full cost of the prior
             read if it overlaps nothing"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))

REPEATS = 5


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def parent_wgrad(path):
    """lmx_op_gemm_wgrad of another build of the library, called positionally (the signature this tree keeps)."""
    from llava_mi355x import _C
    lib = ctypes.CDLL(os.path.abspath(path))
    fn = lib.lmx_op_gemm_wgrad
    fn.restype, fn.argtypes = _C._SIGS["lmx_op_gemm_wgrad"]
    def call(dy, x, out):
        rc = fn(_C.torch_dtype_code(dy.dtype), _C.ptr(dy), dy.stride(0), _C.ptr(x), x.stride(0), dy.shape[0], dy.shape[1], x.shape[1], _C.ptr(out), out.stride(0),
                _C.stream_handle())
        assert rc == 0, "parent lmx_op_gemm_wgrad failed"
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=32768)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--jsonl", default=None)
    args = ap.parse_args()
    from llava_mi355x import ops
    rows = args.rows
    dev = torch.device("cuda:0")
    parent = parent_wgrad(args.parent_lib) if args.parent_lib else None
    med = statistics.median
    spread = lambda v: max(v) - min(v)
    for name, O, I in (("q|k|v", 12288, 4096), ("o_proj", 4096, 4096), ("gate / up", 11008, 4096), ("down", 4096, 11008), ("lm_head", 32000, 4096)):
        dy = (torch.randn((rows, O), device=dev) * 0.1).to(torch.bfloat16)
        x = (torch.randn((rows, I), device=dev) * 0.1).to(torch.bfloat16)
        out = torch.empty((O, I), dtype=torch.bfloat16, device=dev)
        out2 = torch.empty_like(out)
        acc = torch.zeros((O, I), dtype=torch.bfloat16, device=dev)
        fl = 2.0 * rows * O * I
        t = {"plain": [], "acc": [], "parent": [], "copy": []}
        for _ in range(REPEATS):                                   # the variants alternate inside every repeat
            if parent is not None:
                t["parent"].append(timed(lambda: parent(dy, x, out2)))
            t["plain"].append(timed(lambda: ops.gemm_wgrad(dy, x, out)))
            acc.zero_()                                            # 6 accumulations per repeat from zero: the values stay far from the 16-bit range's end
            t["acc"].append(timed(lambda: ops.gemm_wgrad(dy, x, acc, accumulate=True)))
            t["copy"].append(timed(lambda: out2.copy_(out)))
        same_as_parent = None
        if parent is not None:
            parent(dy, x, out2)
            same_as_parent = bool(torch.equal(out, out2))
        us_tr = timed(lambda: (ops.transpose_padded(dy, 64), ops.transpose_padded(x, 64)))
        dyt, xt = ops.transpose_padded(dy, 64), ops.transpose_padded(x, 64)
        us_nt = timed(lambda: ops.gemm(dyt, xt, out=out2))
        bit_identical = bool(torch.equal(out, out2))
        us_direct, us_acc, us_copy = med(t["plain"]), med(t["acc"]), med(t["copy"])
        nbytes = 2.0 * O * I
        copy_rate = 2 * nbytes / us_copy                           # bytes per us, the copy's read + write
        read_us = nbytes / copy_rate
        margin = spread(t["parent"]) if parent is not None else spread(t["plain"])
        rec = {"linear": name, "rows": rows, "out": O, "in": I, "direct_us": round(us_direct, 1), "direct_TFs": round(fl / us_direct / 1e6, 1),
               "plain_spread_us": round(spread(t["plain"]), 1), "acc_us": round(us_acc, 1), "acc_spread_us": round(spread(t["acc"]), 1),
               "acc_minus_plain_us": round(us_acc - us_direct, 1), "copy_us": round(us_copy, 1), "copy_GBs": round(copy_rate / 1e3, 1), "read_us": round(read_us, 1),
               "acc_ok": bool(us_acc <= us_direct + read_us + margin)}
        if parent is not None:
            rec.update({"parent_us": round(med(t["parent"]), 1), "parent_spread_us": round(spread(t["parent"]), 1),
                        "plain_ok": bool(us_direct <= med(t["parent"]) + spread(t["parent"])), "same_bits_as_parent": same_as_parent})
        rec.update({"transposes_us": round(us_tr, 1), "nt_gemm_us": round(us_nt, 1), "nt_gemm_TFs": round(fl / us_nt / 1e6, 1),
                    "old_path_us": round(us_tr + us_nt, 1), "speedup": round((us_tr + us_nt) / us_direct, 3), "bit_identical": bit_identical})
        line = json.dumps(rec)
        print(line, flush=True)
        if args.jsonl:
            os.makedirs(os.path.dirname(os.path.abspath(args.jsonl)), exist_ok=True)
            with open(args.jsonl, "a") as f:
                f.write(line + "\n")
        del dy, x, out, out2, acc, dyt, xt


if __name__ == "__main__":
    main()
