"""TEST INFRASTRUCTURE ONLY -- goldens of the ResNet backbone forward from the UNMODIFIED reference classes on the CPU (needs the reference
tree):
    python -B tools/make_golden_backbone.py [case ...]      tests/golden/backbone_<case>.npz (or backbone_<case>__<layer>.npz, see below)
For every case of tests/backbone_cases.CASES the reference's own `ResNet` -- ltr/models/backbone/resnet.py, or resnet_mrcnn.py for a spec
with `mrcnn` -- is constructed with the case's block class, block counts and `inplanes`, loaded `strict=True` with the seeded parameters of
`backbone_cases.params`, put in eval mode and called with the case's image and output list: in fp32 with f64_bound.THREADS threads, as the
other goldens' fp32 runs, and in float64.  torchvision is absent: the one name the files import from it, `model_urls`, is the harness's
stub.  Keys: tests/backbone_cases.py.  A case whose file would pass 1 MB is written as one file per output.  Every output's maximum has to
lie within [1e-2, 1e2] (the parameter ranges of the case table are chosen for that).  From tests/backbone_np.py only `keys` (through
`params`) is used: no function of the restatement is called here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_harness  # noqa: E402

ref_harness.install()

import backbone_cases as C  # noqa: E402
import f64_bound  # noqa: E402

OUT = os.environ.get("BACKBONE_GOLDEN_OUT", os.path.join(ROOT, "tests", "golden"))
LIMIT = 1000 * 1000


def reference_net(case):
    """the unmodified reference class of the case, parameters loaded strictly, eval mode, fp32"""
    from ltr.models.backbone import resnet, resnet_mrcnn
    spec = case["spec"]
    mod = resnet_mrcnn if spec["mrcnn"] else resnet
    net = mod.ResNet(getattr(mod, spec["kind"]), spec["blocks"], case["outputs"], inplanes=spec["inplanes"])
    return net


def run(name):
    case = C.CASES[name]
    net = reference_net(case)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in C.params(name).items()}, strict=True)
    net.eval()
    x = torch.from_numpy(C.image(name))
    ambient = torch.get_num_threads()
    with torch.no_grad():
        torch.set_num_threads(f64_bound.THREADS)
        try:
            f32 = net(x)
        finally:
            torch.set_num_threads(ambient)
        f64 = net.double()(x.double())
    assert list(f32) == list(f64) == [o for o in C.ALL if o in case["outputs"]], (list(f32), case["outputs"])
    per_output = {}
    for o in f64:
        a64, a32 = f64[o].numpy(), f32[o].numpy()
        assert a64.dtype == np.float64 and a32.dtype == np.float32
        top = float(np.abs(a64).max())
        assert 1e-2 <= top <= 1e2, (name, o, top)
        pos = C.subset(name, o, a64.size)
        per_output[o] = {f"{o}_f64": a64.reshape(-1)[pos], f"{o}_f32": a32.reshape(-1)[pos], f"{o}_shape": np.array(a64.shape),
                         f"{o}_ref_err": np.float64(np.abs(a32.astype(np.float64) - a64).max()), f"{o}_max": np.float64(top),
                         f"{o}_sum": np.float64(a64.sum()), f"{o}_abssum": np.float64(np.abs(a64).sum())}
        print(f"{name:18s} {o:7s} {str(tuple(a64.shape)):20s} max {top:9.3e}  fp32 err {float(per_output[o][o + '_ref_err']):9.3e}")
    total = sum(v.nbytes for d in per_output.values() for v in d.values())
    if total <= LIMIT - 4096:
        files = {f"backbone_{name}.npz": {k: v for d in per_output.values() for k, v in d.items()}}
    else:
        files = {f"backbone_{name}__{o}.npz": d for o, d in per_output.items()}
    for fname, d in files.items():
        path = os.path.join(OUT, fname)
        np.savez(path, **d)
        assert os.path.getsize(path) < LIMIT, (path, os.path.getsize(path))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    for case_name in sys.argv[1:] or list(C.CASES):
        run(case_name)
