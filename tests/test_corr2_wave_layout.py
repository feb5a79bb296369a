"""k_corr2's wave layout for sample pairs of 5-tile maps (DiMP-50: 18x18, n = 50; csrc/fast_passes.hip: pt_fast_plan, `mix`).

The ten (sample, tile) waves of a pair workgroup sat 3 / 3 / 2 / 2 on the CU's four SIMDs with both leftover-carrying tile-0 waves on the
three-wave SIMDs.  The layout that ships splits tile 0 of each sample by positions over two waves (all k-steps each): 12 waves, one half
wave and two full waves per SIMD.  Every element still runs through one accumulator in the same order, so EVERY score keeps its bits
(the k-step split the layout was first built with moved the elements of tile 0 in the last bits and lost on time: profiles/r07a_*).

CPU part: the plan (DiMP-50 new, PrDiMP-50 / ATOM / unpaired DiMP as before) and the shipped instantiations' registers and LDS from
the code object's metadata.  GPU part: the pass and the frame at 50 x 512 x 18 x 18 against the float64 oracle, and bit-equality with the
generic k_corr route (8 channel slices of 16 k-steps through one accumulator per tile, the same shift-and-add order: bit for bit what the
10-wave pair workgroup computed, profiles/r07a_*)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytracking_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LLVM = "/opt/rocm/lib/llvm/bin"
sys.path.insert(0, ROOT)

FIELDS = ("ok", "tiles", "nh", "spw", "mix", "threads", "NK", "KSC", "lds", "left")


def _plan(n, C, H, W, K=4):
    from pytracking_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int * 10)()
    assert L.pt_corr_pass_plan(n, C, H, W, K, K, H + 1 - K % 2, W + 1 - K % 2, out) == 0
    return dict(zip(FIELDS, out))


def test_dimp50_plan_is_the_mixed_pair_layout():
    """18x18, n = 50, C = 512: 5 tiles + leftover quads, two samples per workgroup, 2 * 5 + 2 = 12 waves, every wave sized for all 16
    k-steps of the XCD's 64 channels, one tap-plane set per sample: LDS as before the split."""
    p = _plan(50, 512, 18, 18)
    assert p == dict(ok=1, tiles=5, nh=1, spw=2, mix=1, threads=768, NK=16, KSC=8, lds=(64 * 16 + 2 * 16 * 388) * 4, left=1), p
    # the other channel counts of the pair path, and an odd count (no pairs: k-step halves for every tile)
    assert _plan(64, 256, 18, 18) == dict(p, NK=8, lds=(32 * 16 + 2 * 16 * 388) * 4)
    assert _plan(34, 128, 18, 18) == dict(p, NK=4, lds=(16 * 16 + 2 * 16 * 388) * 4)
    assert _plan(51, 512, 18, 18) == dict(p, nh=2, spw=1, mix=0, threads=640, NK=8)
    assert _plan(32, 512, 18, 18) == dict(p, nh=2, spw=1, mix=0, threads=640, NK=8)


def test_other_geometries_keep_their_plans():
    """PrDiMP-50 (22x22: 8 tiles, one wave each with all k-steps, 8 waves = 2 per SIMD already) and ATOM's 64-channel samples (one
    channel range, k-step halves) come out exactly as before; 3x3 filters on pairs keep the plain 10-wave pair."""
    assert _plan(50, 512, 22, 22) == dict(ok=1, tiles=8, nh=1, spw=1, mix=0, threads=512, NK=16, KSC=8,
                                          lds=(64 * 16 + 16 * 516 + (484 + 2 * 22 + 2 - 516)) * 4, left=0)
    for n in (16, 50, 250):
        assert _plan(n, 64, 18, 18) == dict(ok=1, tiles=5, nh=2, spw=1, mix=0, threads=640, NK=8, KSC=1,
                                            lds=(64 * 16 + 2 * 16 * 388) * 4, left=1), n
    p3 = _plan(50, 512, 18, 18, K=3)
    assert (p3["spw"], p3["nh"], p3["mix"], p3["threads"]) == (2, 1, 0, 640), p3


def test_shipped_mixed_instantiations_fit_their_budget(tmp_path):
    """From the code object's metadata: every k_corr2<NK, LEFT, FUSE, true, 1, MIX = true> uses no scratch and <= 128 VGPRs (the launch
    bound of 4 waves per SIMD; the 12-wave workgroup puts 3 on each), allows the 768-thread block, and its static LDS plus the plan's
    dynamic LDS stays under the 64 KB that need no opt-in (one workgroup per CU at n = 50, a second one wherever 8 n / 2 > 256)."""
    import yaml
    for tool in (HIPCC, os.path.join(LLVM, "clang-offload-bundler"), os.path.join(LLVM, "llvm-readelf")):
        if not os.path.exists(tool):
            pytest.skip(tool + " not available")
    from pytracking_amd import _lib
    obj, co = str(tmp_path / "fast_passes.o"), str(tmp_path / "fast_passes.co")
    r = subprocess.run([HIPCC, *[f for f in _lib.HIPCC_FLAGS if f != "-fPIC"], "--cuda-device-only", "-c", "-I", CSRC, "-I",
                        os.path.join(ROOT, "include"), os.path.join(CSRC, "fast_passes.hip"), "-o", obj], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + obj,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    i = notes.index("amdhsa.kernels")
    doc = notes[notes.rindex("---", 0, i):]
    doc = doc[:doc.index("\n...")]
    kernels = {k[".name"]: k for k in yaml.safe_load(doc)["amdhsa.kernels"]}
    mixed = {name: k for name, k in kernels.items() if re.search(r"7k_corr2ILi\d+ELb[01]ELin?\d+ELb1ELi1ELb1EE", name)}
    # NK in {4, 8, 16} x leftover tile or not x FUSE in {-1, 0, 8, 16}
    assert len(mixed) == 24, sorted(mixed)
    assert any("7k_corr2ILi16ELb1ELi8ELb1ELi1ELb1EE" in name for name in mixed)       # DiMP-50's solver pass
    dyn = {4: 128, 8: 256, 16: 512}
    for name, k in mixed.items():
        nk = int(re.search(r"k_corr2ILi(\d+)E", name).group(1))
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, (name, k[".vgpr_count"], k.get(".agpr_count"))
        assert k[".max_flat_workgroup_size"] >= 768, name
        lds = k[".group_segment_fixed_size"] + _plan(50, dyn[nk], 18, 18)["lds"]
        assert lds <= 64 * 1024, (name, lds)


# ------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------
N, C, H, W, K = 50, 512, 18, 18, 4


def _problem(seed):
    from pytracking_amd import synth
    rng = np.random.default_rng(seed)
    feat = synth.clf_features(rng, N, C, H, W, K)
    filt = rng.standard_normal((C, K, K), dtype=np.float32) * np.float32(0.5 / np.sqrt(C * K * K))
    return feat, filt


@pytest.mark.gpu
def test_apply_filter_dimp50_against_oracle():
    """pt_apply_filter_f32 at 50 x 512 x 18 x 18 (mixed pair workgroups) against the float64 oracle, the project's 1e-4 bound."""
    import torch
    from pytracking_amd import filter as F
    from oracle import np_oracle as O
    feat, filt = _problem(7001)
    got = F.corr_raw(torch.from_numpy(feat).to("cuda:0"), torch.from_numpy(filt).to("cuda:0")).cpu().numpy()
    want = O.apply_filter(feat.astype(np.float64), filt.astype(np.float64))
    err = float(np.abs(got - want).max())
    print(f"apply_filter 50x512x18x18: max abs err {err:.3e} (scores up to {float(np.abs(want).max()):.3f})")
    assert got.shape == want.shape and err < 1e-4, err


@pytest.mark.gpu
def test_every_element_keeps_its_bits():
    """The position split leaves every element on one accumulator, so the elements of unsplit tiles AND of tile 0 are bit-equal to the
    single-accumulator result, produced here by the generic k_corr route (a feature pointer that is not 16-byte aligned takes it): the
    same 8 x 64-channel slices, 16 k-steps through one accumulator per tile, the same shift-and-add and slice-sum order."""
    import torch
    from pytracking_amd import filter as F
    feat, filt = _problem(7002)
    dev = "cuda:0"
    fl = torch.from_numpy(filt).to(dev)
    buf = torch.zeros(feat.size + 4, device=dev)
    al = buf[:feat.size].view(N, C, H, W)
    al.copy_(torch.from_numpy(feat))
    assert al.data_ptr() % 16 == 0
    fast = F.corr_raw(al, fl).cpu().numpy()
    buf2 = torch.zeros(feat.size + 4, device=dev)
    mis = buf2[1:feat.size + 1].view(N, C, H, W)
    mis.copy_(torch.from_numpy(feat))
    assert mis.data_ptr() % 16 == 4
    gen = F.corr_raw(mis, fl).cpu().numpy()
    diff = fast.view(np.int32) != gen.view(np.int32)
    print(f"bitwise differences: {int(diff.sum())} of {diff.size} elements; max abs difference {float(np.abs(fast - gen).max()):.3e}")
    assert np.abs(gen).max() > 0 and not diff.any()


@pytest.mark.gpu
def test_frame_dimp50_fused_gradient_pass_against_oracle():
    """The DiMP-50 frame at n = 50, C = 512 -- the correlation with the fused gradient reduction (FUSE = 8), the memory insert riding
    on the first pass and the plain pass, all on mixed pair workgroups -- against the float64 oracle composition, 1e-4."""
    import torch
    from pytracking_amd import bench_frame, synth
    from oracle import frame_port
    cfg = dict(synth.DIMP50)
    assert (cfg["C"], cfg["H"], cfg["W"], cfg["K"]) == (C, H, W, K)
    for slot in (0, 17):                                            # first / second sample of a pair; slot 0's pair also publishes g
        st = bench_frame.TrackState(cfg, N, seed=311, device="cuda:0")
        x = synth.clf_features(np.random.default_rng(312 + slot), 1, C, H, W, K)[0]
        mem0, bb0, w0 = st.mem_feat.cpu().numpy().copy(), st.mem_bb.cpu().numpy().copy(), st.filter.cpu().numpy().copy()
        st.step(torch.from_numpy(x).to("cuda:0"), slot=slot, num_iter=3)
        torch.cuda.synchronize()
        ref = frame_port.oracle_step(cfg, mem0, bb0, st.sample_weight.cpu().numpy(), w0, x, slot=slot, num_iter=3)
        err_s = float(np.abs(st.scores.cpu().numpy() - ref["scores"]).max())
        err_w = float(np.abs(st.filter.cpu().numpy() - ref["filter"]).max())
        print(f"frame n=50 slot={slot}: score err {err_s:.3e}, filter err {err_w:.3e}")
        assert err_s < 1e-4 and err_w < 1e-4, (slot, err_s, err_w)
        assert np.array_equal(st.mem_feat.cpu().numpy(), ref["mem"])
