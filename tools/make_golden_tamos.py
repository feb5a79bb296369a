"""Golden vectors of the TaMOs multi-object filter predictor from the UNMODIFIED reference: `GOTFilterPredictor` with the reference's
`Transformer` (ltr/models/transformer/{filter_predictor,transformer}.py) and the multi-filter `LinearFilterClassifier`
(ltr/models/transformer/heads.py), imported through oracle.ref_harness, on the cases of tests/tamos_cases.py, in fp32 and in float64.

    python tools/make_golden_tamos.py            # writes tests/golden/tamos_<case>.npz (each well under 1 MiB)

Per case: both filter sets (or the one of predict_filter), the classifier's T score maps, a fixed stride of the encoded maps -- fp32
(`*_f32`) and float64 (`*_f64`) --, the stride, and the predictor's state_dict key names.  Parameters and inputs are not stored: they are
regenerated from the seeds of tests/tamos_cases.py.

The fp32 run is the reference as it stands.  The float64 run is the same modules after `.double()` with one substitution, stated here
because it is the only one: PositionEmbeddingSine evaluates its sines in fp32 whatever the module's dtype (position_encoding.py:52-53),
so the float64 run is handed the float64 table of oracle.tomp_oracle.posenc -- the restatement the existing ToMP golden pins to that
module -- through `get_positional_encoding`.  Otherwise its "float64" output would carry the fp32 sine's 6e-8.

The reference adds the label / box encodings into a view of the caller's `train_feat` when there is one memory frame; every run gets
its own copy.  Test infrastructure: runs on the CPU, needs the reference tree; nothing under tests/ imports it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness                 # noqa: E402
from oracle import tomp_oracle as TO           # noqa: E402
import tamos_cases as TC                       # noqa: E402

ENC_KEEP = 4096                                # encoded-map values stored per output: every ceil(size / ENC_KEEP)-th, flat order


def enc_stride(n):
    return max(1, -(-n // ENC_KEEP))


def build(cfg, params, dtype):
    import ltr.models.transformer.filter_predictor as fp
    import ltr.models.transformer.heads as heads
    import ltr.models.transformer.transformer as trans
    tr = trans.Transformer(d_model=cfg["D"], nhead=cfg["nhead"], num_encoder_layers=cfg["n_enc"], num_decoder_layers=cfg["n_dec"],
                           dim_feedforward=cfg["ff"])
    pred = fp.GOTFilterPredictor(tr, feature_sz=cfg["feature_sz"], num_tokens=cfg["T"], label_enc="gaussian", box_enc="ltrb_token")
    cls = heads.LinearFilterClassifier(num_channels=cfg["D"])
    pred.load_state_dict(TC.state_dict(params, "fp."), strict=True)
    cls.load_state_dict(TC.state_dict(params, "cls."), strict=True)
    pred, cls = pred.eval(), cls.eval()
    if dtype == torch.float64:
        pred, cls = pred.double(), cls.double()

        def pos64(feat):
            nframes, nseq, C, h, w = feat.shape
            t = torch.from_numpy(TO.posenc(h, w, C, cfg["feature_sz"], np.float64))
            return t.t().reshape(1, 1, C, h, w).expand(nframes, nseq, C, h, w)
        pred.get_positional_encoding = pos64
    return pred, cls


def run(name, dtype):
    cfg, params, inputs = TC.case(name)
    pred, cls = build(cfg, params, dtype)
    tr, te, lb, lt = [torch.from_numpy(a.copy()).to(dtype) for a in inputs]
    T = cfg["T"]
    with torch.no_grad():
        if cfg["mode"] == "parallel":
            cw, bw, ce, be = pred.predict_cls_bbreg_filters_parallel(tr, te, lb, cfg["num_gth_frames"], lt)
            out = dict(cls_filter=cw.reshape(1, T, -1), bbreg_filter=bw.reshape(1, T, -1), cls_enc=ce, bbreg_enc=be, scores=cls(ce, cw))
        else:
            w, enc = pred.predict_filter(tr, te, lb, lt)
            out = dict(filter=w.reshape(cfg["n_seq"], T, -1), enc=enc, scores=cls(enc, w))
    return {k: v.numpy() for k, v in out.items()}, list(pred.state_dict().keys())


def main():
    ref_harness.install()
    torch.manual_seed(0)
    gdir = os.path.join(ROOT, "tests", "golden")
    for name in (sys.argv[1:] or TC.CASES):
        store = {}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            out, keys = run(name, dtype)
            for k, v in out.items():
                assert v.dtype == (np.float32 if tag == "f32" else np.float64), (k, v.dtype)
                if k.endswith("enc"):
                    store[f"{k}_stride"] = np.int64(enc_stride(v.size))
                    v = v.reshape(-1)[::enc_stride(v.size)]
                store[f"{k}_{tag}"] = np.ascontiguousarray(v)
        store["state_dict_keys"] = np.array(keys)
        path = os.path.join(gdir, f"tamos_{name}.npz")
        np.savez(path, **store)
        worst = max(float(np.abs(store[k].astype(np.float64) - store[k[:-3] + "f64"]).max()) for k in store if k.endswith("_f32"))
        print(f"{name}: {os.path.getsize(path)} bytes, max |fp32 - float64| {worst:.3e}", flush=True)
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
