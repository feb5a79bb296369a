"""The stride-2 head kernel (tomp.hip: k_gemm_s2) in the compiled gfx950 code object, checked without a GPU (hipcc cross-compiles): its
metadata shows no scratch (private segment) and no spilled registers, and its LDS is the two double-buffered 32 x 68 tiles of the
32 x 32 x 64 GEMM kernel it restates -- four workgroups per CU.  The helpers are those of tests/test_isa_properties.py."""
import os
import subprocess

import pytest

import test_isa_properties as ISA


def _notes(tmp_path_factory):
    import yaml
    for tool in (ISA.HIPCC, os.path.join(ISA.LLVM, "clang-offload-bundler"), os.path.join(ISA.LLVM, "llvm-readelf")):
        if not os.path.exists(tool):
            pytest.skip(tool + " not available")
    from pytracking_amd import _lib
    d = tmp_path_factory.mktemp("feat_head_meta")
    obj, co = str(d / "tomp.o"), str(d / "tomp.co")
    r = subprocess.run([ISA.HIPCC, *[f for f in _lib.HIPCC_FLAGS if f != "-fPIC"], "--cuda-device-only", "-c", "-I", ISA.CSRC, "-I",
                        os.path.join(ISA.ROOT, "include"), os.path.join(ISA.CSRC, "tomp.hip"), "-o", obj], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(ISA.LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + obj,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    notes = subprocess.run([os.path.join(ISA.LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    i = notes.index("amdhsa.kernels")
    doc = notes[notes.rindex("---", 0, i):]
    return {k[".name"]: k for k in yaml.safe_load(doc[:doc.index("\n...")])["amdhsa.kernels"]}


def test_stride_2_head_kernel_has_no_scratch(tmp_path_factory):
    meta = _notes(tmp_path_factory)
    hit = {k: v for k, v in meta.items() if "9k_gemm_s2" in k}
    assert len(hit) == 1, list(meta)
    for name, k in hit.items():
        print(f"\n{name}: private_segment {k['.private_segment_fixed_size']}, vgpr {k['.vgpr_count']} (+ {k.get('.agpr_count', 0)} agpr), "
              f"sgpr {k['.sgpr_count']}, lds {k['.group_segment_fixed_size']}")
        assert int(k[".private_segment_fixed_size"]) == 0, (name, k)
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, (name, k)
        assert int(k[".group_segment_fixed_size"]) == 2 * 2 * 32 * 68 * 4, (name, k)
        assert int(k[".max_flat_workgroup_size"]) == 256 and int(k[".vgpr_count"]) + int(k.get(".agpr_count", 0)) <= 128, (name, k)
    # the kernels the head shares with the stride-1 route keep theirs
    for needle in ("16k_nchw_to_tokens", "11k_gn_reduce", "13k_head_finish"):
        for name, k in meta.items():
            if needle in name:
                assert int(k[".private_segment_fixed_size"]) == 0, (name, k)
