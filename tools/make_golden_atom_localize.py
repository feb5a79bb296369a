"""TEST INFRASTRUCTURE ONLY -- goldens of ATOM's per-frame score localisation from the UNMODIFIED reference on the CPU (needs the reference
tree):
    python -B tools/make_golden_atom_localize.py            tests/golden/atom_localize_<case>.npz
For every case of tests/atom_localize_cases.CASES a bare `ATOM` object (atom_localize_cases.bare_tracker: ATOM.__new__, attributes set by
hand) and the reference's own `localize_target` on it (pytracking/tracker/atom/atom.py:304-406), with torch.rfft / torch.irfft supplied by
tests/eco_shim.py (which tests/test_eco_cpu.py checks against a dense float64 DFT).  Each case runs twice: in float32 as deployed, and in
float64 (float64 inputs and torch's default dtype float64, so that the method's own `torch.Tensor(...)` calls are float64 too).
    flag, scale_ind          the method's returns
    tv, max1                 translation_vec and the maximum of the returned map of the chosen scale, fp32 run
    map                      the returned map of the chosen scale, fp32 run (kept for the small grids and for the case `deployed`)
    tv64, max164, map64      the same of the float64 run (the map for the small grids only)
    ref_fp32_err             per output of atom_localize_np.FLOAT_OUTPUTS: max |fp32 run - float64 run| (max2 is not a return of the method:
                             it takes the map's figure)
Inputs are regenerated from the seeds of the case table by the tests; nothing of the numpy restatement is read here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import eco_shim  # noqa: E402

eco_shim.install()

import atom_localize_cases as C  # noqa: E402

OUT = os.environ.get("ATOM_LOCALIZE_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
FLAG_CODE = {None: 0, "hard_negative": 1, "uncertain": 2, "not_found": 3}


def reference(case, dtype):
    torch.set_default_dtype(dtype)
    try:
        trk = C.bare_tracker(case, dtype=dtype)
        tv, scale_ind, s, flag = trk.localize_target(torch.from_numpy(case["scores"].copy()).to(dtype))
    finally:
        torch.set_default_dtype(torch.float32)
    return tv, int(scale_ind), s, flag


def case_golden(name, case):
    tv, si, s, flag = reference(case, torch.float32)
    tv64, si64, s64, flag64 = reference(case, torch.float64)
    assert (si, flag) == (si64, flag64) and s.dtype == torch.float32 and s64.dtype == torch.float64 and tv64.dtype == torch.float64
    m, m64 = s[si, 0].numpy(), s64[si64, 0].numpy()
    err_map = float(np.abs(s.numpy().astype(np.float64) - s64.numpy()).max())
    err_tv = float(np.abs(tv.numpy().astype(np.float64) - tv64.numpy()).max())
    err_max = abs(float(m.max()) - float(m64.max()))
    g = dict(flag=np.int64(FLAG_CODE[flag]), scale_ind=np.int64(si), tv=tv.numpy(), tv64=tv64.numpy(), max1=np.float32(m.max()), max164=np.float64(m64.max()),
             map_shape=np.array(s.shape), ref_fp32_err=np.array([err_map, err_max, err_map, err_tv]))
    if m.size <= C.STORE_MAP64_CELLS or name == "deployed":
        g["map"] = m
    if m.size <= C.STORE_MAP64_CELLS:
        g["map64"] = m64
    return g


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, case in C.CASES.items():
        g = case_golden(name, case)
        np.savez_compressed(os.path.join(OUT, f"atom_localize_{name}.npz"), **g)
        print(f"{name:28s} flag {int(g['flag'])} scale {int(g['scale_ind'])} tv {g['tv'].tolist()} max1 {float(g['max1']):.6f} "
              f"ref_fp32_err {g['ref_fp32_err'].tolist()}")


if __name__ == "__main__":
    main()
