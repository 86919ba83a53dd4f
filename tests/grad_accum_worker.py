"""One data-parallel rank of the gradient-accumulation ZeRO-2 test (run by test_grad_accum_step_gpu.py): usage grad_accum_worker.py rank world port out.pt"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "llava-plus-codebase_amd"))


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    import torch.distributed as dist
    from synthetic import recipes as synth
    from test_train_step_gpu import build_step, make_batch
    res = {"rank": rank}
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        group = dist.new_group(backend="gloo")
        cfg = synth.CONFIGS["tiny"]
        wnp = synth.make_weights(cfg, 0)
        batches = [make_batch(cfg, seed=0), make_batch(cfg, seed=1)]
        from oracle import llava_oracle as O
        w = O.to_torch_weights(wnp)
        with torch.no_grad():
            towers = [O.vision_tower(w, cfg, b[3]) for b in batches]
        micro = [(b[0], b[2], b[1], t) for b, t in zip(batches, towers)]            # forward_backward's order: ids, labels, mask, features
        kw = dict(lr=1e-3, weight_decay=0.0, max_grad_norm=1.0, bucket_elems=1 << 16)
        single = build_step(cfg, wnp, torch.float32, "cuda:0", **kw)
        single.accumulate_step(micro)
        res["single_params"] = single.flat_p.detach().cpu().clone()
        res["single_norm"] = single.grad_norm()
        # both ranks run the same two micro-batches: the averaged gradients are the single-rank accumulated ones
        from llava_mi355x.train import ZeroPartition
        calls, real = [], ZeroPartition.reduce_scatter
        def counted(self, flat_g, g_shard, b, *a, **k):
            calls.append(b)
            return real(self, flat_g, g_shard, b, *a, **k)
        ZeroPartition.reduce_scatter = counted
        try:
            z = build_step(cfg, wnp, torch.float32, "cuda:0", group=group, **kw)
            z.forward_backward(*micro[0], micro=(0, 2))
            res["scatters_after_micro0"] = list(calls)
            z.forward_backward(*micro[1], micro=(1, 2))
            res["scatters_after_micro1"] = list(calls)
            z.optimizer_step()
            res["scatters_after_step"] = list(calls)
        finally:
            ZeroPartition.reduce_scatter = real
        res["params"] = z.flat_p.detach().cpu().clone()
        res["norm"] = z.grad_norm()
        res["n_buckets"] = len(z.part.buckets)
        res["ok"] = True
    except Exception:  # noqa: BLE001
        import traceback
        res["ok"] = False; res["trace"] = traceback.format_exc()[-2500:]
    torch.save(res, out)
    try:
        dist.barrier(); dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        pass


if __name__ == "__main__":
    main()
