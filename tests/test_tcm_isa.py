"""The target-candidate matching kernels (tcm.hip) keep their state in registers and LDS: no scratch for any of them, and the
descriptor pass's 16 weight vectors stay within a VGPR budget that admits two of its 256-thread workgroups per SIMD set."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytracking_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_tcm_kernels_have_no_scratch(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    sys.path.insert(0, ROOT)
    from pytracking_amd import _lib
    cmd = [HIPCC, *[f for f in _lib.HIPCC_FLAGS if f != "-fPIC"], "--cuda-device-only", "-c", "-I", CSRC, "-I",
           os.path.join(ROOT, "include"), os.path.join(CSRC, "tcm.hip"), "-o", str(tmp_path / "tcm.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        for key, pat in (("vgpr", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = {"k_tcm_peaks", "k_tcm_desc", "k_tcm_desc_combine", "k_tcm_kenc", "k_tcm_linear", "k_tcm_attn", "k_tcm_sinkhorn"}
    found = {n for n in names if any(n in k and re.search(n + r"[^_a-z]", k) for k in res)}
    assert found == names, names - found
    for k, v in res.items():
        assert v["scratch"] == 0, (k, v)
    desc = [v for k, v in res.items() if re.search(r"k_tcm_desc[^_]", k)]
    assert desc and desc[0]["vgpr"] <= 128, desc
