"""--lora_enable through the training entry (llava_mi355x/train_entry.py: train; the reference's scripts/v1_5/finetune_lora.sh -> llava/train/train.py:873-889,
987-997) on the tiny synthetic model and dataset of tests/test_train_entry_gpu.py: the directory it writes is an un-merged LoRA checkpoint that this package's own
load_pretrained_model(dir, base, "...lora...") loads, and the loaded model is the step's merged model."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ckpt_util import write_clip, write_llava  # noqa: E402
from test_train_entry_gpu import _args, _world  # noqa: E402

pytestmark = pytest.mark.gpu


def _margs(D, cfg, tower_name):
    return D.ModelArguments(model_name_or_path="synthetic", version="v1", vision_tower=tower_name, mm_vision_select_layer=cfg.mm_vision_select_layer,
                            mm_projector_type=cfg.mm_projector_type, mm_use_im_start_end=False, mm_use_im_patch_token=False)


def test_lora_training_writes_a_directory_the_loader_merges(cuda, tmp_path):
    from llava_mi355x import conversation as C, train_data as D, train_entry as E
    from llava_mi355x.builder import load_pretrained_model
    from synthetic import build as harness, recipes as synth
    cfg, lc, weights, tok, tower, data_args, model = _world(tmp_path)
    wnp = synth.make_weights(cfg, 0)
    clip_dir = str(tmp_path / "clip-tiny")
    write_clip(clip_dir, cfg, wnp, "4.31")
    base = str(tmp_path / "vicuna-tiny")
    write_llava(base, cfg, wnp, clip_dir, with_projector=False)
    before = {k: v.clone() for k, v in weights.items()}
    targs = _args(D, tmp_path, lora_enable=True, lora_r=8, lora_alpha=16, lora_dropout=0.0, max_steps=2, learning_rate=2e-3, mm_projector_lr=2e-4)
    targs.output_dir = str(tmp_path / "llava-tiny-lora")
    keep = C.default_conversation
    try:
        out = E.train(_margs(D, cfg, clip_dir), data_args, targs, config=lc, weights=weights, tokenizer=tok, vision_tower=tower)
    finally:
        C.default_conversation = keep
    assert out["steps"] == 2 and all(np.isfinite(out["losses"]))
    d = targs.output_dir
    for f in ("adapter_config.json", "adapter_model.safetensors", "non_lora_trainables.bin", "config.json"):
        assert os.path.exists(os.path.join(d, f)), f
    ac = json.load(open(os.path.join(d, "adapter_config.json")))
    assert ac["r"] == 8 and ac["lora_alpha"] == 16 and ac["peft_type"] == "LORA"
    nlt = torch.load(os.path.join(d, "non_lora_trainables.bin"), map_location="cpu", weights_only=True)
    assert nlt and all(k.startswith("base_model.model.model.mm_projector.") for k in nlt)
    ts = out["train_step"]
    for k, v in ts.base.items():                                  # the base did not move; the adapters and the projector did
        assert torch.equal(v.cpu(), before[k].to(v.dtype)), k
    assert any(float(v.abs().max()) > 0 for k, v in ts.lora_state_dict().items() if k.endswith("lora_B.weight"))
    pw = ts.proj_names[0]
    assert not torch.equal(ts.p[pw].cpu(), before["model." + pw])
    # ---- the loader's model against the step's merged model (both merged in fp32 by builder.merge_lora) ----
    tokenizer, loaded, _, _ = load_pretrained_model(d, base, "llava-tiny-lora", torch_dtype=torch.float32)
    merged = dict(wnp)
    merged.update({k: v.float().cpu().numpy() for k, v in ts.merged_state_dict().items()})
    direct = harness.build_model(cfg, dtype=torch.float32, weights=merged)
    n_vocab = len(tokenizer)
    ids_np = synth.make_prompt(cfg, 12, image_positions=(5,))
    ids_np[ids_np >= 0] %= n_vocab
    ids = torch.from_numpy(ids_np)[None].to(cuda)
    pix = torch.from_numpy(synth.make_pixels(cfg, 1)).to(cuda)
    a = loaded.forward(input_ids=ids, images=pix, use_cache=False).logits
    b = direct.forward(input_ids=ids, images=pix, use_cache=False).logits[..., :n_vocab]
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_lora_dropout_bias_and_bits_are_refused(cuda, tmp_path):
    from llava_mi355x import conversation as C, train_data as D, train_entry as E
    cfg, lc, weights, tok, tower, data_args, model = _world(tmp_path)
    keep = C.default_conversation
    try:
        for kw in (dict(lora_dropout=0.05), dict(lora_dropout=0.0, lora_bias="all"), dict(lora_dropout=0.0, bits=4)):
            with pytest.raises(NotImplementedError):
                E.train(_margs(D, cfg, "synthetic-clip"), data_args, _args(D, tmp_path, lora_enable=True, lora_r=8, **kw), config=lc, weights=weights, tokenizer=tok,
                        vision_tower=tower)
    finally:
        C.default_conversation = keep
