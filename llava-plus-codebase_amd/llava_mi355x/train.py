"""One visual-instruction-tuning step on the MI355X kernels (BASELINE config 5).

What the reference runs per step (llava/train/train.py:805-1000 -> HF Trainer.training_step -> LlavaLlamaForCausalLM.forward with labels,
llava_llama.py:56-99; attention through llava/train/llama_flash_attn_monkey_patch.py:68-91; DeepSpeed ZeRO-2 per scripts/zero2.json:16-22;
AdamW, max_grad_norm 1.0 from the HF TrainingArguments defaults the launch scripts keep) and what stands here:

    forward     splice plan (the same lmx_splice_plan as inference: llava_arch.py:99-240) -> packed rows of all samples (the varlen form of
                flash_attn_unpadded_qkvpacked_func: no pad positions are computed) -> decoder layers on the forward kernels (GEMM, RMSNorm,
                RoPE + causal flash attention per sample, SiLU*mul) -> lm_head -> shifted cross-entropy with IGNORE_INDEX
    backward    csrc/train.hip: CE, RMSNorm, SwiGLU, RoPE, attention backward; dgrad / wgrad on the forward GEMM kernels (operands transposed
                once); embedding scatter-add; projector bias / GELU gradients.  The CLIP tower is frozen (clip_encoder.py:25): its features
                come in as data.
    optimiser   global grad-norm clip + AdamW on fp32 master weights and moments (csrc/train.hip adamw_kernel)
    ZeRO-2      ZeroPartition: parameters and gradients live in ONE flat buffer each, laid out in backward order and cut into buckets;
                a bucket whose gradients are complete is reduce-scattered while the backward pass continues (rank r keeps slice r of every
                bucket and the optimiser state for it only), updated slices are all-gathered back.  Collectives are torch.distributed
                (backend "nccl" = RCCL on the GPUs, one process per GPU); with a gloo group (CPU tests, single-GPU dry runs) device tensors
                are staged through the host.

This is the parity-first version: fp32-engine runs match torch autograd + torch.optim.AdamW on the oracle (tests/test_train_step_gpu.py).
`checkpoint=True` keeps only each layer's input and recomputes the layer in the backward pass (the reference's gradient_checkpointing).
`keep_layers` / `keep_budget_bytes` (round 6): with 288 GB per GPU the LAST k layers keep their activations anyway — as many as the budget holds — and are
not recomputed: every kept layer takes one forward (a quarter of its GEMM FLOPs) out of the step; gradients are the same bits either way.

Gradient accumulation (the reference's --gradient_accumulation_steps; HF Trainer divides each micro-batch's mean loss by the count and torch adds into .grad):
forward_backward(..., micro=(i, n)) is micro-batch i of n, accumulate_step(batches) the whole update.  Micro-batch 0 overwrites the gradients, every later one adds
to them INSIDE the kernels that produce them (csrc/gemm8t.hip's accumulating epilogue, the reducer of csrc/lora.hip, cast_f32_add): the prior 16-bit value joins
the fp32 sum and the result is rounded once, so the 16-bit gradient buffer takes one rounding per micro-batch where torch's `.grad += T(new)` takes two (T(new), then
the sum), and no gradient buffer is read and written a second time.  There is no fp32 accumulation buffer.  Buckets are reduce-scattered in the last micro-batch only.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _C, ops
from ._C import check, lib
from .constants import IGNORE_INDEX


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


LORA_PAD = 64                     # adapters are stored with the rank padded to this (the K quantum of the GEMMs, the rank widths of csrc/lora.hip)
LORA_MODULES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")   # module order


@dataclass
class LoraConfig:
    """peft's LoraConfig as the reference fills it (llava/train/train.py:873-889): rank, alpha, the decoder linears that get an adapter.  The default targets are what
    find_all_linear_names (train.py:174-187) yields for this model: every decoder linear, no lm_head, nothing multimodal.  dropout: peft's lora_dropout, the
    probability with which an element of an adapter's input is zeroed (the reference's scripts run 0.05, train.py:113); 0 <= dropout < 1, realised as
    round(dropout * 65536) / 65536 by the counter-based mask of dropout.py."""
    r: int
    alpha: float
    target_modules: Tuple[str, ...] = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
    use_rslora: bool = False
    dropout: float = 0.0

    def __post_init__(self):
        if not 0.0 <= float(self.dropout) < 1.0:
            raise ValueError(f"LoraConfig.dropout must be in [0, 1) (got {self.dropout})")

    @property
    def scaling(self) -> float:
        return float(self.alpha) / math.sqrt(self.r) if self.use_rslora else float(self.alpha) / self.r


def lora_unpad(name: str, t: torch.Tensor, r: int) -> torch.Tensor:
    """The stored (rank-padded) factor -> what peft holds: lora_A [Rp, in] -> [r, in], lora_B [out, Rp] -> [out, r]."""
    return (t[:r] if name.endswith("lora_A.weight") else t[:, :r]).detach().clone()


# ---------------------------------------------------------------------------------------------------------------------------------------
# ZeRO-2 bookkeeping + collectives (no kernels: runs on any device, covered by a gloo world_size-2 test on CPU)
# ---------------------------------------------------------------------------------------------------------------------------------------
class ZeroPartition:
    """Flat layout of named parameters, cut into buckets; rank r owns slice r of every bucket.

    sizes: [(name, numel)] in the order gradients become final (backward order).  Every parameter starts at a multiple of `align`
    elements (16-byte rows for the GEMMs); a bucket closes at the first parameter boundary past `bucket_elems` and is padded so that it
    splits evenly over `world` ranks.  rate_of (name -> learning rate): a bucket also closes where the rate changes, so no bucket mixes two rates and
    `bucket_rate[b]` is the rate of all of bucket b (None without rate_of)."""

    def __init__(self, sizes: Sequence[Tuple[str, int]], world: int = 1, rank: int = 0, bucket_elems: int = 1 << 24, align: int = 64,
                 no_close_after: Sequence[str] = (), rate_of: Optional[Callable[[str], float]] = None):
        assert world >= 1 and 0 <= rank < world
        self.world, self.rank, self.align = int(world), int(rank), int(align)
        self.offset: Dict[str, int] = {}
        self.numel: Dict[str, int] = {}
        self.bucket_of: Dict[str, int] = {}
        self.buckets: List[Tuple[int, int]] = []
        self.members: List[List[str]] = []
        self.bucket_rate: List[Optional[float]] = []
        pos, start, names = 0, 0, []
        hold = set(no_close_after)
        quantum = self.world * self.align
        rate = None
        for name, n in sizes:
            nxt = None if rate_of is None else float(rate_of(name))
            if names and nxt != rate:                           # a rate boundary: the open bucket ends here
                assert names[-1] not in hold, f"learning rates change inside a fused operand at {name}"
                pos = start + _round_up(pos - start, quantum)
                self.buckets.append((start, pos)); self.members.append(names); self.bucket_rate.append(rate)
                start, names = pos, []
            rate = nxt
            self.offset[name], self.numel[name] = pos, int(n)
            self.bucket_of[name] = len(self.buckets)
            names.append(name)
            pos = _round_up(pos + int(n), self.align)
            # a bucket never closes after a name in `no_close_after`: its padding (a multiple of world * align elements, not of the next tensor's
            # row size for world = 3, 5, 6, 7) would separate tensors the step uses as ONE operand (q | k | v)
            if pos - start >= bucket_elems and name not in hold:
                pos = start + _round_up(pos - start, quantum)
                self.buckets.append((start, pos)); self.members.append(names); self.bucket_rate.append(rate)
                start, names = pos, []
        if names:
            pos = start + _round_up(pos - start, quantum)
            self.buckets.append((start, pos)); self.members.append(names); self.bucket_rate.append(rate)
        self.total = pos
        self.shard_offset = []                      # where bucket b's owned slice sits in this rank's shard buffers
        acc = 0
        for s, e in self.buckets:
            self.shard_offset.append(acc)
            acc += (e - s) // self.world
        self.shard_elems = acc

    def owned(self, b: int) -> Tuple[int, int]:
        s, e = self.buckets[b]
        n = (e - s) // self.world
        return s + self.rank * n, s + (self.rank + 1) * n

    def shard_view(self, shard: torch.Tensor, b: int) -> torch.Tensor:
        s, e = self.buckets[b]
        n = (e - s) // self.world
        return shard[self.shard_offset[b]: self.shard_offset[b] + n]

    # ---- collectives ----------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _host_staged(group) -> bool:
        import torch.distributed as dist
        return dist.get_backend(group) == "gloo"

    def reduce_scatter(self, flat_g: torch.Tensor, g_shard: torch.Tensor, b: int, group=None, async_op: bool = False):
        """g_shard's slice for bucket b := sum over ranks of slice `rank` of bucket b of flat_g.  Returns a work handle or None."""
        out = self.shard_view(g_shard, b)
        s, e = self.buckets[b]
        if self.world == 1:
            if out.data_ptr() != flat_g[s:e].data_ptr():          # one rank: the shard buffer may BE the flat buffer (TrainStep does that): nothing to move
                out.copy_(flat_g[s:e])
            return None
        import torch.distributed as dist
        if self._host_staged(group):
            # gloo has no reduce-scatter: all-reduce the bucket on the host and keep the owned slice
            t = flat_g[s:e].float().cpu()
            dist.all_reduce(t, group=group)
            o0, o1 = self.owned(b)
            out.copy_(t[o0 - s: o1 - s].to(out.dtype))
            return None
        return dist.reduce_scatter_tensor(out, flat_g[s:e], group=group, async_op=async_op)

    def all_gather(self, flat_p: torch.Tensor, p_shard: torch.Tensor, b: int, group=None, async_op: bool = False):
        """bucket b of flat_p := concatenation over ranks of their p_shard slices."""
        src = self.shard_view(p_shard, b)
        s, e = self.buckets[b]
        if self.world == 1:
            if src.data_ptr() != flat_p[s:e].data_ptr():
                flat_p[s:e].copy_(src)
            return None
        import torch.distributed as dist
        if self._host_staged(group):
            parts = [torch.empty(src.shape, dtype=src.dtype) for _ in range(self.world)]
            dist.all_gather(parts, src.detach().cpu().contiguous(), group=group)
            flat_p[s:e].copy_(torch.cat(parts).to(flat_p.device))
            return None
        return dist.all_gather_into_tensor(flat_p[s:e], src, group=group, async_op=async_op)

    def all_reduce_scalar(self, x: torch.Tensor, group=None) -> None:
        if self.world == 1:
            return
        import torch.distributed as dist
        if self._host_staged(group) and x.is_cuda:
            t = x.cpu(); dist.all_reduce(t, group=group); x.copy_(t)
        else:
            dist.all_reduce(x, group=group)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------------------------
class TrainStep:
    """Trainable LLM + mm_projector of one LLaVA model on one rank of a data-parallel group.

    config: the LlavaConfig fields the inference model reads (hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
    num_key_value_heads, rms_norm_eps, vocab_size, rope theta, mm_projector_type, mm_hidden_size).  weights: HF-named tensors of the LLM
    and the projector (`model.mm_projector.*` or `mm_projector.*`)."""

    def __init__(self, config, weights: Mapping[str, torch.Tensor], dtype=torch.bfloat16, device="cuda", lr=2e-5, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=1.0, group=None, bucket_elems: Optional[int] = None, checkpoint: bool = False, max_positions: int = 2048,
                 keep_layers: int = 0, keep_budget_bytes: Optional[int] = None, direct_wgrad: bool = True, attn_streams: int = 4,
                 lora: Optional[LoraConfig] = None, lr_for: Optional[Callable[[str], float]] = None, train_base: Sequence[str] = (), lora_seed: int = 0,
                 dropout_seed: Optional[int] = None):
        """lora: train rank-r adapters on the decoder linears instead of the base weights (see the LoRA section below); train_base: base tensors that stay
        trainable next to the adapters and the projector (`lm_head.weight`, `model.norm.weight`, `model.embed_tokens.weight`); lora_seed: seed of the CPU generator
        the A factors are drawn from.  lr_for: name -> learning rate (as in self.p); None: self.lr for everything.  With lr_for, self.lr acts as the schedule's
        base: bucket b steps with lr_for(name) * self.lr / the lr given here.  dropout_seed: the 64-bit key of the LoRA dropout masks (default: lora_seed);
        self.dropout_step counts the forward_backward calls that drew masks (every training call) and is the masks' step counter (settable: the same seed and step give the same masks)."""
        from .model import _projector_kind, _rope_theta
        self.config, self.dtype, self.device = config, dtype, torch.device(device)
        self.lr, self.betas, self.eps, self.wd, self.max_grad_norm = float(lr), tuple(betas), float(eps), float(weight_decay), float(max_grad_norm)
        self.checkpoint = bool(checkpoint)
        self.keep_layers, self.keep_budget_bytes = int(keep_layers), keep_budget_bytes
        self.last_kept_layers = 0
        self._kv_pairs: Dict = {}
        self.attn_streams = int(attn_streams)    # side streams the per-sample attention launches of a layer spread over (0 / 1: the step's stream only)
        self._side: List = []
        self.direct_wgrad = bool(direct_wgrad)   # weight gradients straight from dy / x (csrc/gemm8t.hip) where the shapes allow; False: the two-transpose path
        self.group = group
        self.world, self.rank = 1, 0
        if group is not None:
            import torch.distributed as dist
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        c = config
        self.H, self.I, self.L, self.V = c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.vocab_size
        self.nh = c.num_attention_heads
        self.nkv = getattr(c, "num_key_value_heads", None) or self.nh
        self.D = self.H // self.nh
        self.rms_eps = float(c.rms_norm_eps)
        self.kmult = 64 if dtype in (torch.bfloat16, torch.float16) else 16          # GEMM contraction quantum (csrc/gemm.hip)
        assert self.H % 64 == 0 and self.I % 64 == 0 and self.V % 8 == 0, "hidden / intermediate sizes must be multiples of 64"
        kind, depth = _projector_kind(getattr(c, "mm_projector_type", "linear"))
        self.proj_names: List[str] = []                                                # identity: nothing to train
        if kind == _C.PROJ_LINEAR:
            self.proj_names = ["mm_projector.weight", "mm_projector.bias"]
        elif kind == _C.PROJ_MLP_GELU:
            for j in range(depth):
                self.proj_names += [f"mm_projector.{2 * j}.weight", f"mm_projector.{2 * j}.bias"]
        w = {}
        for k, v in weights.items():
            k = k.replace("model.mm_projector.", "mm_projector.")
            w[k] = v
        # ---- flat layout, backward order ---------------------------------------------------------------------------------------------
        order: List[str] = ["lm_head.weight", "model.norm.weight"]
        for l in reversed(range(self.L)):
            p = f"model.layers.{l}."
            order += [p + "mlp.down_proj.weight", p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", p + "post_attention_layernorm.weight",
                      p + "self_attn.o_proj.weight", p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight",
                      p + "input_layernorm.weight"]
        for j in reversed(range(len(self.proj_names) // 2)):
            order += [self.proj_names[2 * j + 1], self.proj_names[2 * j]]
        order.append("model.embed_tokens.weight")
        missing = [n for n in order if n not in w]
        if missing:
            raise KeyError(f"weights missing for the trainable part: {missing[:4]}...")
        self.shapes = {n: tuple(w[n].shape) for n in order}
        if bucket_elems is None:
            bucket_elems = self.H * self.H                       # DeepSpeed's "auto" reduce_bucket_size = hidden_size^2
        # q | k | v of a layer form one fused operand of the step: no bucket boundary (padding) between them, whatever the world size
        fused = [f"model.layers.{l}.self_attn.{p}_proj.weight" for l in range(self.L) for p in ("q", "k")]
        nq = (self.nh + 2 * self.nkv) * self.D
        self.lora, self.lr_for, self.base_lr = lora, lr_for, float(lr)
        self.dropout_seed = int(lora_seed if dropout_seed is None else dropout_seed)
        self.dropout_step = 0                                    # advanced by every forward_backward call that draws masks (a micro-batch), not by the optimiser
        self._drop_on = True                                     # False inside a forward_backward(dropout=False) call: the adapters see x itself
        self._drop_step = 0                                      # the step of the call that is running: recomputed layers and the backward read the same one
        self.lora_mods: Tuple[str, ...] = ()
        self._sB: Optional[Dict[str, torch.Tensor]] = None       # LoRA: scaling * B per adapter, valid until the parameters change
        self.base: Dict[str, torch.Tensor] = {}                  # LoRA: the frozen base tensors, outside the flat buffers
        self.p: Dict[str, torch.Tensor] = {}
        self.g: Dict[str, torch.Tensor] = {}
        self.qkv_w, self.qkv_g = [], []
        flat_order = order
        if lora is not None:
            # ---- LoRA: only the adapters, the projector and `train_base` are parameters of the optimiser; the base lives in plain device tensors ----------
            assert lora.r >= 1 and float(lora.alpha) > 0
            self.lora_mods = tuple(m for m in LORA_MODULES if m.split(".")[1] in set(lora.target_modules))
            unknown = set(lora.target_modules) - {m.split(".")[1] for m in LORA_MODULES}
            if unknown or not self.lora_mods:
                raise ValueError(f"LoRA target modules {sorted(unknown) or list(lora.target_modules)}: only the decoder linears {[m.split('.')[1] for m in LORA_MODULES]} take adapters")
            extra = set(train_base)
            if extra - {"lm_head.weight", "model.norm.weight", "model.embed_tokens.weight"}:
                raise ValueError("train_base: only lm_head.weight, model.norm.weight and model.embed_tokens.weight can train next to the adapters")
            self.Rp = _round_up(lora.r, LORA_PAD)
            in_out = {"self_attn.q_proj": (self.H, self.nh * self.D), "self_attn.k_proj": (self.H, self.nkv * self.D), "self_attn.v_proj": (self.H, self.nkv * self.D),
                      "self_attn.o_proj": (self.nh * self.D, self.H), "mlp.gate_proj": (self.H, self.I), "mlp.up_proj": (self.H, self.I), "mlp.down_proj": (self.I, self.H)}
            groups = (("mlp.down_proj",), ("mlp.gate_proj", "mlp.up_proj"), ("self_attn.o_proj",), ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"))
            flat_order = [n for n in ("lm_head.weight", "model.norm.weight") if n in extra]
            fused = []
            self.lora_groups: Dict[Tuple[int, str], Tuple[str, ...]] = {}            # (layer, first module of a group that shares its input) -> the group's targets
            for l in reversed(range(self.L)):
                for grp in groups:
                    ts = tuple(m for m in grp if m in self.lora_mods)
                    if not ts:
                        continue
                    self.lora_groups[(l, grp[0])] = ts
                    a_names = [f"model.layers.{l}.{m}.lora_A.weight" for m in ts]
                    flat_order += a_names + [f"model.layers.{l}.{m}.lora_B.weight" for m in ts]
                    fused += a_names[:-1]                                            # the A factors of a group are ONE stacked operand: no padding between them
                    for m in ts:
                        self.shapes[f"model.layers.{l}.{m}.lora_A.weight"] = (self.Rp, in_out[m][0])
                        self.shapes[f"model.layers.{l}.{m}.lora_B.weight"] = (in_out[m][1], self.Rp)
            for j in reversed(range(len(self.proj_names) // 2)):
                flat_order += [self.proj_names[2 * j + 1], self.proj_names[2 * j]]
            if "model.embed_tokens.weight" in extra:
                flat_order.append("model.embed_tokens.weight")
            for l in range(self.L):
                pre = f"model.layers.{l}.self_attn."
                qkv = torch.empty((nq, self.H), dtype=dtype, device=self.device)     # q | k | v stay one fused operand: allocated as one
                at = 0
                for pn in ("q_proj", "k_proj", "v_proj"):
                    rows = self.shapes[pre + pn + ".weight"][0]
                    self.base[pre + pn + ".weight"] = qkv[at:at + rows]; at += rows
                self.qkv_w.append(qkv); self.qkv_g.append(None)
            for n in order:
                if n not in flat_order:
                    if n not in self.base:
                        self.base[n] = torch.empty(self.shapes[n], dtype=dtype, device=self.device)
                    self.base[n].copy_(w[n].to(device=self.device, dtype=dtype))
        rate_of = None if lr_for is None else (lambda n: float(lr_for(n)))
        self.part = ZeroPartition([(n, int(np.prod(self.shapes[n]))) for n in flat_order], self.world, self.rank, bucket_elems, no_close_after=fused, rate_of=rate_of)
        P = self.part
        self.flat_p = torch.zeros(P.total, dtype=dtype, device=self.device)
        self.flat_g = torch.zeros(P.total, dtype=dtype, device=self.device)
        for n in flat_order:
            o, k = P.offset[n], P.numel[n]
            self.p[n] = self.flat_p[o:o + k].view(self.shapes[n])
            self.g[n] = self.flat_g[o:o + k].view(self.shapes[n])
            if n in w:
                self.p[n].copy_(w[n].to(device=self.device, dtype=dtype))
        if lora is None:
            # q | k | v rows are adjacent in the flat buffer: one fused [(nh + 2 nkv) D, H] operand without a copy
            for l in range(self.L):
                o = P.offset[f"model.layers.{l}.self_attn.q_proj.weight"]
                assert P.offset[f"model.layers.{l}.self_attn.k_proj.weight"] == o + self.nh * self.D * self.H
                assert P.offset[f"model.layers.{l}.self_attn.v_proj.weight"] == o + (self.nh + self.nkv) * self.D * self.H
                self.qkv_w.append(self.flat_p[o:o + nq * self.H].view(nq, self.H))
                self.qkv_g.append(self.flat_g[o:o + nq * self.H].view(nq, self.H))
        else:
            self.p.update(self.base)                             # self.p resolves every name: the forward reads base and trainable tensors the same way
            # peft's initialisation (LoraLayer.reset_lora_parameters): A = kaiming_uniform_(a = sqrt(5)), i.e. U(-1 / sqrt(in), 1 / sqrt(in)), drawn on the CPU
            # in module order; B = 0.  Rows of A / columns of B past r are zero and stay zero (their gradients are products with zero columns; weight decay is 0).
            gen = torch.Generator().manual_seed(int(lora_seed))
            self.lora_A_stack: Dict[Tuple[int, str], torch.Tensor] = {}
            for l in range(self.L):
                for m in self.lora_mods:
                    a = self.p[f"model.layers.{l}.{m}.lora_A.weight"]
                    draw = torch.empty((lora.r, a.shape[1]), dtype=torch.float32)
                    bound = 1.0 / math.sqrt(a.shape[1])
                    draw.uniform_(-bound, bound, generator=gen)
                    a[:lora.r].copy_(draw.to(dtype))
            for (l, first), ts in self.lora_groups.items():
                o = P.offset[f"model.layers.{l}.{ts[0]}.lora_A.weight"]
                k_in = self.shapes[f"model.layers.{l}.{ts[0]}.lora_A.weight"][1]
                for i, m in enumerate(ts):
                    assert P.offset[f"model.layers.{l}.{m}.lora_A.weight"] == o + i * self.Rp * k_in
                self.lora_A_stack[(l, first)] = self.flat_p[o:o + len(ts) * self.Rp * k_in].view(len(ts) * self.Rp, k_in)
        # ---- optimiser state for the owned slices only (ZeRO-2) -----------------------------------------------------------------------
        n_own = P.shard_elems
        self.master = torch.empty(n_own, dtype=torch.float32, device=self.device)
        for b in range(len(P.buckets)):
            o0, o1 = P.owned(b)
            P.shard_view(self.master, b).copy_(self.flat_p[o0:o1].float())
        self.exp_avg = torch.zeros(n_own, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros(n_own, dtype=torch.float32, device=self.device)
        if self.world == 1:
            # one rank owns every bucket whole and the shard layout IS the flat layout: the "shards" are the flat buffers themselves — no reduce-scatter / all-gather
            # stand-in copies (2 x 13.5 GB moved per 7B step) and 27 GB less resident, which the kept-activation budget turns into five more layers
            assert n_own == P.total and all(P.shard_offset[b] == P.buckets[b][0] for b in range(len(P.buckets)))
            self.g_shard, self.p_shard = self.flat_g, self.flat_p
        else:
            self.g_shard = torch.zeros(n_own, dtype=dtype, device=self.device)
            self.p_shard = torch.zeros(n_own, dtype=dtype, device=self.device)
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.step_count = 0
        self.last_grad_norm: Optional[float] = None
        # ---- RoPE table, exactly as the inference model builds it ---------------------------------------------------------------------
        theta = _rope_theta(c)
        inv_freq = 1.0 / (theta ** (torch.arange(0, self.D, 2, dtype=torch.int64).to(torch.float32) / self.D))
        freqs = torch.arange(int(max_positions), dtype=torch.float32)[:, None] * inv_freq[None, :]
        self.rope = torch.cat([freqs.cos(), freqs.sin()], dim=-1).contiguous().to(self.device)
        self.max_positions = int(max_positions)
        self._pending: List = []
        self._ready: Dict[int, int] = {}
        self._acc = False                                        # inside a forward_backward call of a micro-batch i > 0: the gradient writers add to self.g
        self._last_micro = True                                  # ... of the last micro-batch of an update: buckets are reduce-scattered as they complete
        self._micro_next: Optional[Tuple[int, int]] = None       # the micro-batch an unfinished accumulation waits for (None: optimizer_step may run)
        self.frozen: set = set()
        self.comm_stream = torch.cuda.Stream(device=self.device) if (self.world > 1 and self.device.type == "cuda") else None

    # ---- helpers ------------------------------------------------------------------------------------------------------------------------
    def _wgrad(self, dy: torch.Tensor, x: torch.Tensor, out: torch.Tensor) -> None:
        """out [N, K] = dy[M, N]^T @ x[M, K]   (M is a multiple of the contraction quantum: the packed rows are padded to it).  In a micro-batch past the first
        (self._acc) the product is added to what `out` holds, in fp32 before the one rounding."""
        if self.direct_wgrad and ops.wgrad_direct_ok(dy, x, out):
            ops.gemm_wgrad(dy, x, out, accumulate=self._acc)         # both operands in their forward layout (csrc/gemm8t.hip): no transposed copies
        else:                                                        # residual = out: every GEMM epilogue reads residual[m][n] in the thread that stores out[m][n]
            ops.gemm(ops.transpose_padded(dy, self.kmult), ops.transpose_padded(x, self.kmult), residual=out if self._acc else None, out=out)

    def _dgrad(self, dy: torch.Tensor, w: torch.Tensor, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dy [M, N] @ w [N, K] -> [M, K] (+ residual)."""
        N = w.shape[0]
        wt = ops.transpose_padded(w, self.kmult)                 # [K, Np]
        if wt.shape[1] != N:
            pad = torch.zeros((dy.shape[0], wt.shape[1]), dtype=dy.dtype, device=dy.device)
            pad[:, :N].copy_(dy)
            dy = pad
        return ops.gemm(dy, wt, residual=residual)

    # ---- LoRA pieces: y = x W^T + scaling (x A^T) B^T per target linear ---------------------------------------------------------------------------
    def _lora_down(self, l: int, first: str, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        """u = x A^T for every target of the group that shares the input x, as ONE GEMM on the stacked A factors; {module: its [rows, Rp] column window of u}."""
        ts = self.lora_groups.get((l, first), ()) if self.lora is not None else ()
        if not ts:
            return {}
        A = self.lora_A_stack[(l, first)]
        if self._drop_on and self.lora.dropout > 0.0:
            # u = dropout_m(x) A_m^T, every adapter under its own mask.  The mask is applied inside csrc/lora.hip's down kernel; where that kernel does not take
            # the call (the fp32 verification step, odd shapes) the masked input is materialised per adapter (ops.dropout) for the plain GEMM.
            Rp, drop = self.Rp, self._drop()
            u = torch.empty((x.shape[0], len(ts) * Rp), dtype=x.dtype, device=x.device)
            sid = [self._drop_stream(l, m) for m in ts]
            if sid == list(range(sid[0], sid[0] + len(ts))) and ops.lora_down_dropout_ok(x, A, len(ts), out=u):
                ops.lora_down_dropout(x, A, len(ts), *drop, sid[0], out=u)
            else:
                for i in range(len(ts)):
                    A_i, u_i = A[i * Rp:(i + 1) * Rp], u[:, i * Rp:(i + 1) * Rp]
                    if ops.lora_down_dropout_ok(x, A_i, 1, out=u_i):
                        ops.lora_down_dropout(x, A_i, 1, *drop, sid[i], out=u_i)
                    else:
                        ops.gemm(ops.dropout(x, *drop, sid[i]), A_i, out=u_i)
        else:
            u = ops.gemm(x, A)
        return {m: u[:, i * self.Rp:(i + 1) * self.Rp] for i, m in enumerate(ts)}

    def _drop_stream(self, l: int, m: str) -> int:
        """The mask stream of one adapter: rank << 16 | layer << 3 | index of the module in LORA_MODULES."""
        from .dropout import stream_id
        return stream_id(self.rank, l, LORA_MODULES.index(m))

    def _drop(self) -> Tuple[float, int, int]:
        return float(self.lora.dropout), self.dropout_seed, self._drop_step

    def lora_keep_mask(self, layer: int, module: str, rows: int, cols: int, step: Optional[int] = None) -> np.ndarray:
        """bool [rows, cols]: which elements of the input of adapter `module` (`q_proj` or `self_attn.q_proj`) of `layer` are kept; rows are the packed rows of this
        rank's block in the order forward_backward packs them (sample after sample, valid positions only).  step: the forward_backward call the mask belongs to;
        None = the next call (self.dropout_step).  All True without dropout."""
        from .dropout import keep_mask
        assert self.lora is not None, "not a LoRA step"
        full = next(m for m in LORA_MODULES if m == module or m.split(".")[1] == module)
        if self.lora.dropout == 0.0:
            return np.ones((int(rows), int(cols)), dtype=bool)
        return keep_mask(self.lora.dropout, self.dropout_seed, self.dropout_step if step is None else int(step), self._drop_stream(layer, full), rows, cols)

    def _lora_sB(self, l: int, m: str) -> torch.Tensor:
        """scaling * B, [out, Rp]: the operand of the up-projection and of du = dy (scaling B).  Built once per optimiser step for all adapters (one pass over the
        flat parameter buffer's copy) and dropped when the parameters change.  Rounded to the model dtype: exact when the scaling is a power of two
        (alpha = 2 r of the reference's scripts), one extra 16-bit rounding of B otherwise (peft rounds the product u B^T instead)."""
        if self._sB is None:
            flat = self.flat_p * self.lora.scaling               # B factors are views into the flat buffer: scale it whole, read the same offsets
            P = self.part
            self._sB = {n: flat[P.offset[n]:P.offset[n] + P.numel[n]].view(self.shapes[n]) for n in self.g if n.endswith("lora_B.weight")}
        return self._sB[f"model.layers.{l}.{m}.lora_B.weight"]

    def _lora_up(self, l: int, m: str, u: torch.Tensor, y: torch.Tensor) -> None:
        """y += u (scaling B)^T in place: the existing GEMM with K = Rp and residual = out = y (a column window of q|k|v through its row stride).  Every GEMM
        epilogue, the split-K reducers included, reads residual[m][n] in the thread that then stores out[m][n], so the two may be the same buffer."""
        ops.gemm(u, self._lora_sB(l, m), residual=y, out=y)

    def _lora_backward(self, l: int, m: str, dy: torch.Tensor, x: torch.Tensor, u: torch.Tensor, into: Optional[torch.Tensor]) -> torch.Tensor:
        """Gradients of one adapter from dy [rows, out], the linear's input x [rows, in] and the stashed u = x A^T; returns `into` + du A ([rows, in]: the adapter's
        share of dx).  du = dy (scaling B); dB = scaling dy^T u; dA = du^T x — the two factor gradients on csrc/lora.hip where it takes the shape.  With dropout, u is
        the stashed dropout(x) A^T and x stands for dropout(x) below; nothing masked was stashed."""
        An, Bn = f"model.layers.{l}.{m}.lora_A.weight", f"model.layers.{l}.{m}.lora_B.weight"
        du = self._dgrad(dy, self._lora_sB(l, m))
        if ops.lora_wgrad_ok(dy, u, self.g[Bn]):
            ops.lora_wgrad(dy, u, self.g[Bn], alpha=self.lora.scaling, accumulate=self._acc)
        else:                                                # the fp32 verification step, odd shapes: the two-transpose path
            self._wgrad(dy, u * self.lora.scaling, self.g[Bn])
        if self._drop_on and self.lora.dropout > 0.0:
            # the adapter saw dropout(x): dA = du^T dropout(x) with the mask regenerated inside the wgrad kernel, and its share of dx is mask * scale * (du A),
            # added to `into` in fp32 (ops.dropout_add takes every dtype of the step; the first adapter of a chain has nothing to add to).  The elementwise forms
            # ask only for columns in multiples of 8 and 16-byte aligned rows (ops.dropout_ok), which the hidden / intermediate sizes (multiples of 64, asserted
            # in __init__) and the step's own buffers always give; there is no other HIP path to fall back to, so anything else is refused here by name.
            assert ops.dropout_ok(x), "LoRA dropout: the adapter input must have columns in multiples of 8 and 16-byte aligned rows"
            drop = (*self._drop(), self._drop_stream(l, m))
            if ops.lora_wgrad_ok(x, du, self.g[An], transposed=True):
                ops.lora_wgrad_dropout(x, du, *drop, out=self.g[An], transposed=True, accumulate=self._acc)
            else:
                self._wgrad(du, ops.dropout(x, *drop), self.g[An])
            t = self._dgrad(du, self.p[An])
            return ops.dropout(t, *drop, out=t) if into is None else ops.dropout_add(into, t, *drop)
        if ops.lora_wgrad_ok(x, du, self.g[An], transposed=True):
            ops.lora_wgrad(x, du, self.g[An], transposed=True, accumulate=self._acc)
        else:
            self._wgrad(du, x, self.g[An])
        return self._dgrad(du, self.p[An], residual=into)

    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        """Un-padded adapter factors, A [r, in] and B [out, r], keyed `model.layers.N.<module>.lora_A.weight` / `.lora_B.weight`."""
        assert self.lora is not None, "not a LoRA step"
        r, out = self.lora.r, {}
        for l in range(self.L):
            for m in self.lora_mods:
                base = f"model.layers.{l}.{m}."
                for f in ("lora_A.weight", "lora_B.weight"):
                    out[base + f] = lora_unpad(base + f, self.p[base + f], r)
        return out

    def load_lora_state_dict(self, state: Mapping[str, torch.Tensor]) -> None:
        """Set adapter factors (un-padded, keys as lora_state_dict gives them) and re-seed the fp32 master copies from them."""
        assert self.lora is not None, "not a LoRA step"
        r = self.lora.r
        for k, v in state.items():
            t = self.p[k]
            (t[:r] if k.endswith("lora_A.weight") else t[:, :r]).copy_(v.to(device=self.device, dtype=self.dtype))
        self._sync_master()

    def merged_state_dict(self) -> Dict[str, torch.Tensor]:
        """The model with every adapter merged, W + scaling B A, in fp32 on the device through builder.merge_lora (what loading the saved adapter gives)."""
        assert self.lora is not None, "not a LoRA step"
        from .builder import merge_lora
        ad = self.lora_state_dict()
        out = {}
        for n, t in self.p.items():
            if ".lora_" in n:
                continue
            mod = n[:-len(".weight")] if n.endswith(".weight") else n
            if mod + ".lora_A.weight" in ad:
                out[n] = merge_lora(t.detach(), ad[mod + ".lora_A.weight"], ad[mod + ".lora_B.weight"], self.lora.scaling, self.device)      # all operands already on the device
            else:
                out[n] = t.detach().float()
        return out

    def _sync_master(self) -> None:
        P = self.part
        self._sB = None
        for b in range(len(P.buckets)):
            o0, o1 = P.owned(b)
            P.shard_view(self.master, b).copy_(self.flat_p[o0:o1].float())

    def _attn_streams(self, n_items: int):
        """Context manager for the per-sample attention launches of one layer: `with self._attn_streams(n) as on: with on(i) as lane: ...` runs item i on side stream
        i % attn_streams (lane = that index; 0 streams or fewer than two items: everything stays on the step's stream, lane 0).  The side streams wait for the step's
        stream on entry and the step's stream waits for all of them on exit.  Why: a 2048-row sample's attention launches are 512 workgroups of very different length
        (1 .. 32 key tiles); run one after the other each launch ends with most CUs idle behind its heaviest workgroups, run side by side the next sample's workgroups
        fill them.  No arithmetic changes (no atomics anywhere: same bits)."""
        import contextlib
        step = self

        class _Ctx:
            def __enter__(self_c):
                self_c.use = step.attn_streams >= 2 and n_items >= 2 and step.device.type == "cuda"
                if self_c.use:
                    while len(step._side) < step.attn_streams:
                        step._side.append(torch.cuda.Stream(device=step.device))
                    self_c.main = torch.cuda.current_stream(step.device)
                    ev = torch.cuda.Event(); ev.record(self_c.main)
                    for s in step._side[:step.attn_streams]:
                        s.wait_event(ev)

                @contextlib.contextmanager
                def on(i):
                    if not self_c.use:
                        yield 0
                    else:
                        k = i % step.attn_streams
                        with torch.cuda.stream(step._side[k]):
                            yield k
                return on

            def __exit__(self_c, *exc):
                if self_c.use:
                    for s in step._side[:step.attn_streams]:
                        self_c.main.wait_stream(s)
                return False
        return _Ctx()

    def _kv_scratch(self, s_max: int, dtype, lane: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
        """K / V^T cache of one sample for the forward attention: a scratch pair per length, zeroed ONCE and reused by every span, layer and step (launches on one
        stream: the next rope_kv overwrites it after the previous flash attention has read it).  Slots past a sample's length hold whatever earlier samples left
        (any values, NaN / Inf included): the kernels mask them, V included.  Allocating zeroed caches per span was 0.5 GB of fills per layer at 16 x 2048."""
        key = (int(s_max), dtype, int(lane))                           # one pair per side stream: samples on different streams run at the same time
        if key not in self._kv_pairs:
            self._kv_pairs[key] = ops.alloc_kv(self.nkv, int(s_max), self.D, dtype, self.device)
        return self._kv_pairs[key]

    @staticmethod
    def _zero_rows_outside(t: torch.Tensor, spans: List[Tuple[int, int]]) -> None:
        """Zero the rows of `t` that no span covers (the padding of the packed rows): the spans' rows are about to be overwritten, a fill of the whole
        buffer (268 - 805 MB per layer at 16 x 2048) is not needed."""
        at = 0
        for a, b in sorted(spans):
            if a > at:
                t[at:a].zero_()
            at = max(at, b)
        if at < t.shape[0]:
            t[at:].zero_()

    def layer_activation_bytes(self, rows: int) -> int:
        """Bytes one decoder layer's stash holds beyond its input rows (what _layer_forward returns: h, q|k|v with q and k rotated, attn, x1, h2, gate, up, act)."""
        es = torch.empty((), dtype=self.dtype).element_size()
        per_row = 3 * self.H + (self.nh + 2 * self.nkv) * self.D + self.nh * self.D + 3 * self.I
        if self.lora is not None:
            per_row += len(self.lora_mods) * self.Rp                       # the stashed u = x A^T of every adapter
        return int(rows) * per_row * es

    def set_trainable(self, predicate) -> None:
        """Freeze every parameter whose name (as in self.p: HF names, the projector as `mm_projector.*`) the predicate rejects — the reference's
        `requires_grad_(False)` (llava/train/train.py:850-851, 925-934: freeze_backbone, tune_mm_mlp_adapter, freeze_mm_mlp_adapter).  A frozen tensor's
        gradient is cleared the moment it is final, before its bucket is reduced: it adds nothing to the clipping norm, its Adam moments stay zero and the
        update leaves its bits unchanged.  (Weight decay would still shrink it: refused.)"""
        frozen = {n for n in self.p if not predicate(n)}
        if frozen and self.wd != 0.0:
            raise ValueError("frozen parameters with weight_decay != 0 are not supported (the reference's scripts train with weight_decay 0.)")
        self.frozen = frozen

    def _mark_ready(self, names: Sequence[str]) -> None:
        """Gradients of `names` are final for this micro-batch: in the LAST micro-batch of an update, reduce-scatter every bucket that just became complete, on the
        communication stream (still under that call's backward); earlier micro-batches only accumulate locally in flat_g."""
        P = self.part
        for n in names:
            if n in self.frozen:
                self.g[n].zero_()
            if not self._last_micro:
                continue
            b = P.bucket_of[n]
            self._ready[b] = self._ready.get(b, 0) + 1
            if self._ready[b] == len(P.members[b]):
                if self.comm_stream is not None:
                    self.comm_stream.wait_stream(torch.cuda.current_stream(self.device))
                    with torch.cuda.stream(self.comm_stream):
                        h = P.reduce_scatter(self.flat_g, self.g_shard, b, self.group, async_op=False)
                else:
                    h = P.reduce_scatter(self.flat_g, self.g_shard, b, self.group)
                self._pending.append(h)

    def _plan(self, input_ids, attention_mask, labels, slot_rows: np.ndarray):
        ids_h = np.ascontiguousarray(input_ids.detach().cpu().numpy().astype(np.int64))
        B, Lq = ids_h.shape
        mask_h = None if attention_mask is None else np.ascontiguousarray(attention_mask.detach().cpu().numpy().astype(np.uint8))
        lab_h = None if labels is None else np.ascontiguousarray(labels.detach().cpu().numpy().astype(np.int64))
        vp = lambda a: ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)
        max_len = getattr(self.config, "tokenizer_model_max_length", None) or 0
        left = getattr(self.config, "tokenizer_padding_side", "right") == "left"
        T = ctypes.c_int32(0)
        args = (vp(ids_h), vp(mask_h), vp(lab_h), B, Lq, 0, vp(slot_rows), len(slot_rows), int(max_len), int(left))
        if lib.lmx_splice_plan(*args, ctypes.byref(T), None, None, None, None):
            raise IndexError(_C.last_error())
        Tn = T.value
        src = np.empty((B, Tn), np.int32); om = np.empty((B, Tn), np.uint8); op = np.empty((B, Tn), np.int64); ol = np.empty((B, Tn), np.int64)
        check(lib.lmx_splice_plan(*args, ctypes.byref(T), vp(src), vp(om), vp(op), vp(ol)), "lmx_splice_plan")
        return src, om.astype(bool), ol

    # ---- forward + backward ---------------------------------------------------------------------------------------------------------------
    def _layer_forward(self, l: int, x: torch.Tensor, spans: List[Tuple[int, int]]):
        p = f"model.layers.{l}."
        W, nh, nkv, D = self.p, self.nh, self.nkv, self.D
        h = ops.rmsnorm(x, W[p + "input_layernorm.weight"], self.rms_eps)
        qkv = ops.gemm(h, self.qkv_w[l])
        us: Dict[str, torch.Tensor] = {}
        us.update(self._lora_down(l, "self_attn.q_proj", h))
        for m, c0, c1 in (("self_attn.q_proj", 0, nh * D), ("self_attn.k_proj", nh * D, (nh + nkv) * D), ("self_attn.v_proj", (nh + nkv) * D, (nh + 2 * nkv) * D)):
            if m in us:
                self._lora_up(l, m, us[m], qkv[:, c0:c1])
        attn = torch.empty((x.shape[0], nh * D), dtype=x.dtype, device=x.device)
        self._zero_rows_outside(attn, spans)                                          # padding rows feed o_proj: finite zeros, as before
        # the forward's log-sum-exp, kept for the backward (FlashAttention-2's statistics); allocated on the step's stream BEFORE the samples spread over the side streams
        # (one allocation for the layer, no fill: rows past a sample's length are never written and only ever read by the key-side kernel's tile staging, which
        # discards them by SELECT, not by a multiplication — tests/test_wgrad_gpu.py runs the backward on a NaN-filled buffer)
        if x.dtype == torch.float32:
            lses = []
        else:
            tp = [_round_up(b - a, 64) for a, b in spans]
            flat = torch.empty(nh * sum(tp), dtype=torch.float32, device=x.device)
            lses, at = [], 0
            for n in tp:
                lses.append(flat[at:at + nh * n].view(nh, n)); at += nh * n
        with self._attn_streams(len(spans)) as on:
            for i, (a, b) in enumerate(spans):
                with on(i) as lane:
                    Tn = b - a
                    kc, vt = self._kv_scratch(_round_up(Tn, 128), x.dtype, lane)
                    rows = qkv[a:b]
                    ops.rope_kv(rows, kc, vt, self.rope, 0, nh, nkv, D, k_rows=True)   # q AND k rotated in place (the backward reads both from qkv), k / v into the caches
                    if x.dtype == torch.float32:  # fp32 verification mode: the VALU attention kernel, as the inference engine's fp32 prefill
                        ops.decode_attn(rows, kc, vt, Tn, 0, 0, nh, nkv, D, True, q_stride=qkv.stride(0), out=attn[a:b])
                    else:
                        ops.flash_attn(rows, kc, vt, Tn, Tn, 0, nh, nkv, D, True, q_stride=qkv.stride(0), out=attn[a:b], lse=lses[i])
        x1 = ops.gemm(attn, W[p + "self_attn.o_proj.weight"], residual=x)
        us.update(self._lora_down(l, "self_attn.o_proj", attn))
        if "self_attn.o_proj" in us:
            self._lora_up(l, "self_attn.o_proj", us["self_attn.o_proj"], x1)
        h2 = ops.rmsnorm(x1, W[p + "post_attention_layernorm.weight"], self.rms_eps)
        gate = ops.gemm(h2, W[p + "mlp.gate_proj.weight"])
        up = ops.gemm(h2, W[p + "mlp.up_proj.weight"])
        us.update(self._lora_down(l, "mlp.gate_proj", h2))
        if "mlp.gate_proj" in us:
            self._lora_up(l, "mlp.gate_proj", us["mlp.gate_proj"], gate)
        if "mlp.up_proj" in us:
            self._lora_up(l, "mlp.up_proj", us["mlp.up_proj"], up)
        act = ops.elementwise(ops.EW_SWIGLU, gate, up)
        x2 = ops.gemm(act, W[p + "mlp.down_proj.weight"], residual=x1)
        us.update(self._lora_down(l, "mlp.down_proj", act))
        if "mlp.down_proj" in us:
            self._lora_up(l, "mlp.down_proj", us["mlp.down_proj"], x2)
        return x2, dict(x=x, h=h, qkv=qkv, attn=attn, lse=lses, x1=x1, h2=h2, gate=gate, up=up, act=act, u=us)

    def _layer_backward(self, l: int, st: dict, d: torch.Tensor, spans: List[Tuple[int, int]]) -> torch.Tensor:
        p = f"model.layers.{l}."
        W, G, nh, nkv, D = self.p, self.g, self.nh, self.nkv, self.D
        dt = _C.torch_dtype_code(d.dtype)
        # MLP: x2 = x1 + down(silu(gate) * up)
        # With LoRA the base wgrads are skipped (the base is not a parameter) and every target linear adds its adapter's gradients and its share of dx (`side`).
        lora = self.lora is not None
        us = st.get("u", {})
        side = lambda m, dy, x, into=None: self._lora_backward(l, m, dy, x, us[m], into) if m in us else into
        d_act = self._dgrad(d, W[p + "mlp.down_proj.weight"], residual=side("mlp.down_proj", d, st["act"]))
        if not lora:
            self._wgrad(d, st["act"], G[p + "mlp.down_proj.weight"])
        dg, du = ops.swiglu_bwd(st["gate"], st["up"], d_act)
        if not lora:
            self._wgrad(dg, st["h2"], G[p + "mlp.gate_proj.weight"])
            self._wgrad(du, st["h2"], G[p + "mlp.up_proj.weight"])
        s2 = side("mlp.up_proj", du, st["h2"], side("mlp.gate_proj", dg, st["h2"]))
        dh2 = self._dgrad(du, W[p + "mlp.up_proj.weight"], residual=self._dgrad(dg, W[p + "mlp.gate_proj.weight"], residual=s2))
        dx1, dw = ops.rmsnorm_bwd(st["x1"], W[p + "post_attention_layernorm.weight"], dh2, self.rms_eps, want_dw=not lora, residual=d)     # d joins over the skip connection
        if not lora:
            ops.cast_f32(dw, G[p + "post_attention_layernorm.weight"], accumulate=self._acc)
        # attention: x1 = x + o_proj(attn)
        d_attn = self._dgrad(dx1, W[p + "self_attn.o_proj.weight"], residual=side("self_attn.o_proj", dx1, st["attn"]))
        if not lora:
            self._wgrad(dx1, st["attn"], G[p + "self_attn.o_proj.weight"])
        qkv = st["qkv"]
        dqkv = torch.empty_like(qkv)
        self._zero_rows_outside(dqkv, spans)
        ld = qkv.stride(0)
        es = qkv.element_size()
        ko, vo = nh * D * es, (nh + nkv) * D * es                                     # byte offsets of the k / v columns inside a q|k|v row
        with self._attn_streams(len(spans)) as on:
            for i, (a, b) in enumerate(spans):
                with on(i):
                    Tn = b - a
                    rows, dq_rows = qkv[a:b], dqkv[a:b]
                    # q, k (both rotated in place by the forward) and v are column windows of the q|k|v rows; dq, dk, dv go straight into the same windows of dqkv
                    at = lambda t, o: ctypes.c_void_p(t.data_ptr() + o)
                    if st["lse"]:          # 16-bit step: the forward's log-sum-exp and output come in (FlashAttention-2's form): no statistics sweep in the backward
                        lse, o_rows = st["lse"][i], st["attn"][a:b]
                        check(lib.lmx_op_attn_bwd_lse(dt, D, _C.ptr(rows), at(rows, ko), at(rows, vo), _C.ptr(o_rows), _C.ptr(d_attn[a:b]), _C.ptr(lse), lse.stride(0),
                                                      _C.ptr(dq_rows), at(dq_rows, ko), at(dq_rows, vo), Tn, nh, nkv, ld, ld, d_attn.stride(0), o_rows.stride(0),
                                                      1.0 / math.sqrt(D), _C.stream_handle()), "attn_bwd_lse")
                    else:                  # fp32 verification step: the two-pass VALU kernels recompute the statistics
                        s1 = torch.empty(Tn * nkv * D, dtype=torch.float32, device=d.device); s2 = torch.empty_like(s1)
                        check(lib.lmx_op_attn_bwd(dt, D, _C.ptr(rows), at(rows, ko), at(rows, vo), _C.ptr(d_attn[a:b]), _C.ptr(dq_rows), _C.ptr(s1), _C.ptr(s2),
                                                  at(dq_rows, ko), at(dq_rows, vo), Tn, nh, nkv, ld, ld, d_attn.stride(0), 1.0 / math.sqrt(D), _C.stream_handle()),
                              "attn_bwd")
                    # un-rotate dq | dk in place: they are adjacent heads of the same rows
                    check(lib.lmx_op_rope_bwd(dt, _C.ptr(dq_rows), _C.ptr(dq_rows), _C.ptr(self.rope), 0, Tn, nh + nkv, D, ld, _C.stream_handle()), "rope_bwd")
        s3 = None
        for m, c0, c1 in (("self_attn.q_proj", 0, nh * D), ("self_attn.k_proj", nh * D, (nh + nkv) * D), ("self_attn.v_proj", (nh + nkv) * D, (nh + 2 * nkv) * D)):
            s3 = side(m, dqkv[:, c0:c1], st["h"], s3)
        dh = self._dgrad(dqkv, self.qkv_w[l], residual=s3)
        if lora:
            dx, _ = ops.rmsnorm_bwd(st["x"], W[p + "input_layernorm.weight"], dh, self.rms_eps, want_dw=False, residual=dx1)
            self._mark_ready([f"{p}{m}.lora_{f}.weight" for m in self.lora_mods for f in ("A", "B")])
            return dx
        self._wgrad(dqkv, st["h"], self.qkv_g[l])
        dx, dw = ops.rmsnorm_bwd(st["x"], W[p + "input_layernorm.weight"], dh, self.rms_eps, residual=dx1)
        ops.cast_f32(dw, G[p + "input_layernorm.weight"], accumulate=self._acc)
        self._mark_ready([p + "mlp.down_proj.weight", p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", p + "post_attention_layernorm.weight",
                          p + "self_attn.o_proj.weight", p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight",
                          p + "input_layernorm.weight"])
        return dx

    def _projector_forward(self, f: torch.Tensor):
        """f [rows, mm_hidden] (frozen tower features, rows padded to the contraction quantum) -> (features [rows, H], stash)."""
        W = self.p
        if not self.proj_names:
            return f, None
        zs, ins = [], []
        x = f
        n_lin = len(self.proj_names) // 2
        for j in range(n_lin):
            if j > 0:
                zs.append(x)
                x = ops.elementwise(ops.EW_GELU, x)
            ins.append(x)
            x = ops.gemm(x, W[self.proj_names[2 * j]], bias=W[self.proj_names[2 * j + 1]])
        return x, dict(zs=zs, ins=ins)

    def _projector_backward(self, st: Optional[dict], d: torch.Tensor) -> None:
        if st is None:
            return
        W, G = self.p, self.g
        n_lin = len(self.proj_names) // 2
        for j in reversed(range(n_lin)):
            wn, bn = self.proj_names[2 * j], self.proj_names[2 * j + 1]
            self._wgrad(d, st["ins"][j], G[wn])
            ops.cast_f32(ops.col_sum(d), G[bn], accumulate=self._acc)
            if j > 0:
                da = self._dgrad(d, W[wn])
                d = ops.elementwise(ops.EW_GELU_BWD, st["zs"][j - 1], da)
        self._mark_ready(self.proj_names)

    def forward_backward(self, input_ids: torch.Tensor, labels: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                         image_features: Optional[torch.Tensor] = None, slot_rows: Optional[Sequence[int]] = None, backward: bool = True,
                         dropout: Optional[bool] = None, micro: Optional[Tuple[int, int]] = None):
        """One micro-batch.  input_ids / labels / attention_mask: [B, L] (ids carry IMAGE_TOKEN_INDEX markers); image_features: output of the
        frozen tower, [n_images, P, mm_hidden] (or a flat [rows, mm_hidden] with slot_rows = rows per image slot).
        Returns (loss fp32 device scalar, number of counted label positions).  Gradients land in self.g (flat_g).
        dropout (LoraConfig.dropout > 0 only): None = `backward`, i.e. a training call draws its masks and advances self.dropout_step, while a forward-only call
        is an evaluation in peft's sense (nn.Dropout is the identity in eval mode): no masks, and the counter, hence the masks of later training calls, stays
        where it is.  True / False force either (a forward-only look at the training loss; a backward through the unmasked adapters).
        micro = (i, n): this call is micro-batch i of the n that make one optimiser step (gradient accumulation); None = (0, 1).  The loss gradient is scaled by
        1 / (world * n) (HF Trainer divides each micro-batch's mean loss by n; the returned loss is the micro-batch's own mean).  Micro-batch 0 overwrites every
        gradient, micro-batches i > 0 add to self.g inside the gradient kernels (one rounding each); buckets are reduce-scattered in micro-batch n - 1 only, and
        optimizer_step() refuses to run before it."""
        dev, dt = self.device, self.dtype
        mi, mn = (0, 1) if micro is None else (int(micro[0]), int(micro[1]))
        if not (mn >= 1 and 0 <= mi < mn):
            raise ValueError(f"micro = (i, n) needs 0 <= i < n (got {micro})")
        if backward:
            if mi > 0 and self._micro_next != (mi, mn):
                raise RuntimeError(f"micro-batch {mi} of {mn} does not follow the last backward call (expected {self._micro_next or 'a first micro-batch'})")
            self._acc, self._last_micro = mi > 0, mi == mn - 1
            self._micro_next = None if mi == mn - 1 else (mi + 1, mn)
        self._drop_on = bool(backward) if dropout is None else bool(dropout)
        if self._drop_on:
            self._drop_step = self.dropout_step                  # one mask set per micro-batch: micro-batches of one accumulation must not share masks
            self.dropout_step += 1
        if image_features is not None and image_features.dim() == 3:
            slot_rows = [image_features.shape[1]] * image_features.shape[0]
            image_features = image_features.reshape(-1, image_features.shape[-1])
        slot_rows_np = np.ascontiguousarray(np.asarray(slot_rows if slot_rows is not None else [], dtype=np.int32))
        src, valid, lab = self._plan(input_ids, attention_mask, labels, slot_rows_np)
        B, Tn = src.shape
        # ---- pack the valid positions of all samples into one row block (varlen), padded with empty rows to the contraction quantum ----
        spans, rows_src, rows_lab, at = [], [], [], 0
        for b in range(B):
            idx = np.nonzero(valid[b])[0]
            if idx.size == 0:
                continue
            if idx.size > self.max_positions:
                raise ValueError("sequence longer than the RoPE table")
            s, l = src[b, idx], lab[b, idx].copy()
            l[0] = IGNORE_INDEX            # the row before a sample's first token belongs to the previous sample: it predicts nothing
            spans.append((at, at + idx.size)); at += idx.size
            rows_src.append(s); rows_lab.append(l)
        Np = _round_up(max(at, 1), self.kmult)
        src_p = np.full(Np, -1, np.int32); lab_p = np.full(Np, IGNORE_INDEX, np.int64)
        src_p[:at] = np.concatenate(rows_src); lab_p[:at] = np.concatenate(rows_lab)
        src_d = torch.from_numpy(src_p).to(dev); lab_d = torch.from_numpy(lab_p).to(dev)
        # ---- projector on the frozen tower's features, embedding gather + splice ---------------------------------------------------------
        feats, pst, f_rows = None, None, 0
        if image_features is not None:
            f_rows = image_features.shape[0]
            f = torch.zeros((_round_up(f_rows, self.kmult), image_features.shape[1]), dtype=dt, device=dev)
            f[:f_rows].copy_(image_features.to(device=dev, dtype=dt))
            feats, pst = self._projector_forward(f)
        x = ops.gather_embed(src_d, self.p["model.embed_tokens.weight"], feats)
        # ---- decoder ----------------------------------------------------------------------------------------------------------------------
        stash = []
        keep_from = 0
        if self.checkpoint:
            # activations of the LAST layers stay (they are consumed first by the backward): the explicit count, or as many as the byte budget holds
            kept = min(self.L, max(0, self.keep_layers))
            if self.keep_budget_bytes is not None:
                kept = max(kept, min(self.L, int(self.keep_budget_bytes // max(1, self.layer_activation_bytes(Np)))))
            keep_from = self.L - kept
            self.last_kept_layers = kept
        for l in range(self.L):
            x_in = x
            x, st = self._layer_forward(l, x, spans)
            stash.append({"x": x_in} if (self.checkpoint and l < keep_from) else st)
        hn = ops.rmsnorm(x, self.p["model.norm.weight"], self.rms_eps)
        logits = ops.gemm(hn, self.p["lm_head.weight"])
        loss, count, dlogits = ops.ce_loss(logits[None], lab_d[None], ignore_index=IGNORE_INDEX, want_grad=backward, grad=1.0 / self.world if mn == 1 else 1.0 / (self.world * mn))
        if not backward:
            return loss, count
        # ---- backward (gradients of a data-parallel group are averaged: each rank back-propagates loss / world) ---------------------------
        self._ready.clear(); self._pending.clear()
        dlogits = dlogits[0]
        dhn = self._dgrad(dlogits, self.p["lm_head.weight"])
        if "lm_head.weight" in self.g:                           # with LoRA the base is not a parameter: a base tensor has a gradient only if `train_base` names it
            self._wgrad(dlogits, hn, self.g["lm_head.weight"])
        d, dw = ops.rmsnorm_bwd(x, self.p["model.norm.weight"], dhn, self.rms_eps, want_dw="model.norm.weight" in self.g)
        if "model.norm.weight" in self.g:
            ops.cast_f32(dw, self.g["model.norm.weight"], accumulate=self._acc)
        self._mark_ready([n for n in ("lm_head.weight", "model.norm.weight") if n in self.g])
        del logits, dlogits
        for l in reversed(range(self.L)):
            st = stash[l]
            if len(st) == 1:                                     # only the layer's input was kept: recompute it
                _, st = self._layer_forward(l, st["x"], spans)
            d = self._layer_backward(l, st, d, spans)
            stash[l] = None
        want_dE = "model.embed_tokens.weight" in self.g
        dE = torch.zeros((self.V, self.H), dtype=torch.float32, device=dev) if want_dE else None       # LoRA: no [V, H] fp32 table
        dfeats = torch.zeros_like(feats) if (feats is not None and pst is not None) else None
        ops.embed_bwd(src_d, d, dE, dfeats)
        if pst is not None:
            self._projector_backward(pst, dfeats)
        elif self.proj_names:
            if not self._acc:                  # a text-only micro-batch: the projector took no part (an accumulating one adds nothing to what earlier ones left)
                for n in self.proj_names:
                    self.g[n].zero_()
            self._mark_ready(self.proj_names)
        if want_dE:
            ops.cast_f32(dE.view(-1), self.g["model.embed_tokens.weight"].view(-1), accumulate=self._acc)
            self._mark_ready(["model.embed_tokens.weight"])
        return loss, count

    # ---- optimiser ------------------------------------------------------------------------------------------------------------------------
    def optimizer_step(self) -> None:
        """Clip by the global norm of the (averaged) gradients, AdamW on this rank's slices, all-gather the updated parameters."""
        if self._micro_next is not None:
            raise RuntimeError(f"optimizer_step() in the middle of a gradient accumulation: micro-batch {self._micro_next[0]} of {self._micro_next[1]} has not run "
                               "(the gradients are partial and, with more than one rank, not reduced)")
        P = self.part
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        if self.comm_stream is not None:
            cur.wait_stream(self.comm_stream)
        for h in self._pending:
            if h is not None:
                h.wait()
        self._pending.clear()
        self.step_count += 1
        self.gnorm_sq.zero_()
        ops.sumsq(self.g_shard, self.gnorm_sq)                   # padding elements of the shards are zero
        P.all_reduce_scalar(self.gnorm_sq, self.group)
        for b in range(len(P.buckets)):
            view = lambda t: P.shard_view(t, b)
            # lr_for: every bucket holds one rate (ZeroPartition closes buckets at rate boundaries); self.lr / base_lr is the schedule's factor
            lr = self.lr if P.bucket_rate[b] is None else P.bucket_rate[b] * (self.lr / self.base_lr if self.base_lr != 0.0 else 0.0)
            ops.adamw(view(self.p_shard), view(self.g_shard), view(self.master), view(self.exp_avg), view(self.exp_avg_sq), lr, self.betas, self.eps,
                      self.wd, self.step_count, gnorm_sq=self.gnorm_sq if self.max_grad_norm > 0 else None, max_grad_norm=self.max_grad_norm)
            P.all_gather(self.flat_p, self.p_shard, b, self.group)
        self.last_grad_norm = None
        self._sB = None                                          # the parameters moved

    def grad_norm(self) -> float:
        """Global gradient norm of the last step (host read: a sync)."""
        return float(self.gnorm_sq.sqrt().item())

    def accumulate_step(self, batches: Sequence[Sequence]) -> Tuple[torch.Tensor, torch.Tensor]:
        """One optimiser step over len(batches) micro-batches (gradient accumulation): each entry is the argument tuple of forward_backward (input_ids, labels,
        attention_mask, image_features, slot_rows; trailing ones may be left out).  Returns (mean of the micro-batch losses, total counted positions)."""
        n = len(batches)
        if n < 1:
            raise ValueError("accumulate_step needs at least one micro-batch")
        losses, counts = [], []
        for i, args in enumerate(batches):
            loss, count = self.forward_backward(*args, micro=(i, n))
            losses.append(loss); counts.append(count)
        self.optimizer_step()
        return torch.stack(losses).mean(), torch.stack(counts).sum()

    def step(self, input_ids, labels, attention_mask=None, image_features=None, slot_rows=None):
        loss, count = self.forward_backward(input_ids, labels, attention_mask, image_features, slot_rows)
        self.optimizer_step()
        return loss, count

    def trainable_state_dict(self) -> Dict[str, torch.Tensor]:
        """The tensors the optimiser owns (with LoRA: the padded adapter factors, the projector and `train_base`; without: everything)."""
        return {n: self.p[n].detach().clone() for n in self.g}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Every tensor the forward reads, by name (with LoRA: the base as it is, un-merged, and the padded adapter factors)."""
        return {n: t.detach().clone() for n, t in self.p.items()}
