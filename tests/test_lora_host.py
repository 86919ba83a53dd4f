"""Host side of LoRA training (no GPU): the reference's arguments (llava/train/train.py:110-115), the adapter directory the training entry writes
(train.py:987-997: adapter_config.json + adapter_model.safetensors in peft's key form, non_lora_trainables.bin) read back by this package's own loader
(builder.read_lora_adapter, the key rule of llava/model/builder.py:72-74), and the flat ZeRO layout with two learning rates."""
import json
import math
import os

import pytest
import torch


def test_training_arguments_carry_the_reference_lora_fields():
    from llava_mi355x.train_data import TrainingArguments
    t = TrainingArguments()
    assert (t.lora_enable, t.lora_r, t.lora_alpha, t.lora_dropout, t.lora_weight_path, t.lora_bias) == (False, 64, 16, 0.05, "", "none")
    assert t.mm_projector_lr is None


def test_lora_config_scaling_and_default_targets():
    from llava_mi355x.train import LoraConfig
    c = LoraConfig(r=128, alpha=256)
    assert c.scaling == 2.0 and set(c.target_modules) == {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"}
    assert LoraConfig(r=64, alpha=16, use_rslora=True).scaling == 16 / 8.0


@pytest.mark.parametrize("rslora", [False, True])
@pytest.mark.parametrize("r", [8, 128])
def test_saved_adapter_directory_reads_back(tmp_path, r, rslora):
    from llava_mi355x import builder
    from llava_mi355x.train import LORA_PAD, lora_unpad
    from llava_mi355x.train_entry import save_lora_adapter
    g = torch.Generator().manual_seed(r)
    Rp = -(-r // LORA_PAD) * LORA_PAD
    mods = {"model.layers.0.self_attn.q_proj": (48, 32), "model.layers.0.mlp.down_proj": (32, 80), "model.layers.1.self_attn.v_proj": (16, 32)}     # (out, in)
    stored, plain = {}, {}
    for m, (o, i) in mods.items():
        A, B = torch.randn((r, i), generator=g), torch.randn((o, r), generator=g)
        plain[m] = (A, B)
        Ap, Bp = torch.zeros((Rp, i)), torch.zeros((o, Rp))                   # as the step stores them: rank padded to a multiple of 64 with zeros
        Ap[:r], Bp[:, :r] = A, B
        stored[m + ".lora_A.weight"], stored[m + ".lora_B.weight"] = Ap, Bp
    state = {k: lora_unpad(k, v, r) for k, v in stored.items()}
    proj = {"mm_projector.0.weight": torch.randn((32, 24), generator=g), "mm_projector.0.bias": torch.randn(32, generator=g)}
    alpha = 2 * r
    path = save_lora_adapter(str(tmp_path), None, r=r, lora_alpha=alpha, target_modules=("q_proj", "v_proj", "down_proj"), use_rslora=rslora, lora_state=state,
                             non_lora_state=proj)
    assert os.path.basename(path) == "adapter_model.safetensors"
    ac = json.load(open(tmp_path / "adapter_config.json"))
    assert ac["peft_type"] == "LORA" and ac["task_type"] == "CAUSAL_LM" and ac["r"] == r and ac["lora_alpha"] == alpha and ac["bias"] == "none"
    assert ac["use_rslora"] is rslora and sorted(ac["target_modules"]) == ["down_proj", "q_proj", "v_proj"]
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        keys = set(f.keys())
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight" in keys and len(keys) == 2 * len(mods)      # peft's key form, un-padded on disk
    pairs, scaling = builder.read_lora_adapter(str(tmp_path))
    assert scaling == (alpha / math.sqrt(r) if rslora else alpha / r)
    assert set(pairs) == {m + ".weight" for m in mods}
    for m, (A, B) in plain.items():
        gotA, gotB = pairs[m + ".weight"]
        assert tuple(gotA.shape) == (r, mods[m][1]) and tuple(gotB.shape) == (mods[m][0], r)
        assert torch.equal(gotA, A) and torch.equal(gotB, B)
    # non_lora_trainables.bin: the reference's rule (llava/model/builder.py:72-74) leaves checkpoint names
    nlt = torch.load(tmp_path / "non_lora_trainables.bin", map_location="cpu", weights_only=True)
    assert set(nlt) == {"base_model.model.model.mm_projector.0.weight", "base_model.model.model.mm_projector.0.bias"}
    nlt = {(k[11:] if k.startswith("base_model.") else k): v for k, v in nlt.items()}
    if any(k.startswith("model.model.") for k in nlt):
        nlt = {(k[6:] if k.startswith("model.") else k): v for k, v in nlt.items()}
    assert set(nlt) == {"model.mm_projector.0.weight", "model.mm_projector.0.bias"}
    assert torch.equal(nlt["model.mm_projector.0.weight"], proj["mm_projector.0.weight"])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_zero_partition_with_two_rates_keeps_them_in_separate_buckets(world):
    from llava_mi355x.train import ZeroPartition
    sizes = [(f"layers.{l}.{m}.lora_{f}", 64 * 40 if f == "A" else 96 * 64) for l in (1, 0) for m in ("down", "q", "k") for f in ("A", "B")]
    sizes += [("mm_projector.2.bias", 96), ("mm_projector.2.weight", 96 * 96), ("mm_projector.0.bias", 96), ("mm_projector.0.weight", 96 * 24), ("embed", 1000)]
    rate = lambda n: 2e-5 if "mm_projector" in n else 2e-4
    for bucket_elems in (1, 5000, 1 << 24):
        P = ZeroPartition(sizes, world=world, rank=0, bucket_elems=bucket_elems, rate_of=rate)
        assert len(P.bucket_rate) == len(P.buckets) == len(P.members)
        for b, names in enumerate(P.members):
            assert {rate(n) for n in names} == {P.bucket_rate[b]}, names           # one rate per bucket
        assert [n for names in P.members for n in names] == [n for n, _ in sizes]   # order kept, nothing lost
        assert len(P.buckets) >= 3                                                  # adapters | projector | embed: two boundaries at least
        for (s, e) in P.buckets:
            assert (e - s) % (world * P.align) == 0
    plain = ZeroPartition(sizes, world=world, rank=0, bucket_elems=1 << 24)
    assert plain.bucket_rate == [None] and len(plain.buckets) == 1                  # without rates nothing changes
