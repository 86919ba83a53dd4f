"""The rank-r weight-gradient kernel (csrc/lora.hip) must stay free of scratch: its staging registers (two + R / 32 16-byte loads in flight per lane across the
MFMA segment) once sat in scratch as an array of structs, 80 - 176 bytes per lane.  hipcc reports the numbers at compile time; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "llava-plus-codebase_amd", "csrc")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_lora_wgrad_instantiations_have_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I.", "-I../../include", "-c", "lora.hip", "-o", str(tmp_path / "l.o"),
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    main = [k for k in usage if "lora_wgrad_kernel" in k]
    red = [k for k in usage if "lora_wgrad_reduce_kernel" in k]
    assert len(main) == 8 and len(red) == 4, sorted(usage)       # {bf16, f16} x R / 64 in 1 .. 4; {bf16, f16} x {plain, transposed}
    bad = {k: v for k, v in usage.items() if v != 0}
    assert not bad, bad
