"""Shared by tests/test_tamos_cpu.py, tests/test_gpu_tamos.py, tools/make_golden_tamos.py and tools/bench_tamos.py: the configurations
that put the TaMOs multi-object filter predictor (pt_tamos_* of pytracking_amd/csrc/tomp.hip, pytracking_amd/tamos.py) on every kernel
route its launchers can pick and on the shapes where its kernels change path -- one query, a ragged and a full 16-query tile, a memory
that is no multiple of the 64-key chunk, a bbreg row whose leading chunks are nothing but masked keys, more keys than the ToMP decoder
takes, head widths 16 / 32 / 64, up to 8 batch rows, no encoder, one decoder layer -- with, next to every case, the ordered route list
pt_tamos_predict_routes reports and the fp32 restatement's own distance from float64 (tests/tamos_f64.py).  Parameters and inputs are
seeded as tests/tomp_cases.py seeds them; in every case with T >= 3 a middle object is absent (zero labels, zero boxes).  Reads nothing
outside the repository.  Test infrastructure only."""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from pytracking_amd import _lib, synth

R = _lib.TOMP_ROUTES
RT = _lib.TAMOS_ROUTES


def _p(D, nhead, ff, H, W, T, n_train, mode, n_seq=1, gth=0, n_enc=1, n_dec=2):
    assert mode in ("parallel", "filter") and (mode == "filter" or n_seq == 1)
    return dict(D=D, nhead=nhead, ff=ff, n_enc=n_enc, n_dec=n_dec, H=H, W=W, feature_sz=max(H, W), T=T, n_train=n_train,
                num_gth_frames=gth, mode=mode, n_seq=n_seq)


CASES = OrderedDict([
    # ---- base: L = 105 keys is no multiple of 16; then one query, the deployed count, a ragged and a full 16-query tile (T nhead = 44, 64)
    ("base_t3", _p(128, 4, 256, 5, 7, 3, 2, "parallel", gth=1, n_enc=2)),
    ("base_t1", _p(128, 4, 256, 5, 7, 1, 2, "parallel", gth=1, n_enc=2)),
    ("base_t10", _p(128, 4, 256, 5, 7, 10, 2, "parallel", gth=1, n_enc=2)),
    ("base_t11", _p(128, 4, 256, 5, 7, 11, 2, "parallel", gth=1, n_enc=2)),
    ("base_t16", _p(128, 4, 256, 5, 7, 16, 2, "parallel", gth=1, n_enc=2)),
    # ---- the bbreg row: every memory key masked (162 keys: its first two 64-key chunks hold nothing but padding), the deployed
    #      pattern, an empty mask range
    ("mask9_gth0", _p(256, 8, 256, 9, 9, 10, 2, "parallel", gth=0)),
    ("mask9_gth1", _p(256, 8, 256, 9, 9, 10, 2, "parallel", gth=1)),
    ("mask9_gth2", _p(256, 8, 256, 9, 9, 10, 2, "parallel", gth=2)),
    # ---- past the ToMP decoder's key limit (nhead (L + 4) <= 11000): L = 1444, 23 key chunks per row; 2888 rows: the encoder's
    #      128 x 64 tile and split-K routes
    ("keys1444", _p(256, 8, 512, 19, 19, 10, 3, "parallel", gth=1)),
    # ---- head width 16 (L = 1452) and 64; more than two batch rows on blockIdx
    ("head16_keys1452", _p(128, 8, 256, 22, 22, 4, 2, "filter")),
    ("head64_seq3", _p(512, 8, 256, 5, 5, 5, 2, "filter", n_seq=3)),
    ("d384_t3", _p(384, 6, 320, 5, 7, 3, 2, "parallel", gth=1)),
    # ---- one memory frame (the reference writes into its caller's train_feat there); up to 8 batch rows
    ("seq1", _p(128, 4, 256, 5, 5, 3, 1, "filter", n_seq=1)),
    ("seq2", _p(128, 4, 256, 5, 5, 3, 1, "filter", n_seq=2)),
    ("seq8", _p(128, 4, 256, 5, 5, 3, 1, "filter", n_seq=8)),
    # ---- one decoder layer (tgt = 0 throughout the self-attention); no encoder
    ("dec1", _p(128, 4, 256, 5, 7, 3, 2, "parallel", gth=1, n_enc=2, n_dec=1)),
    ("enc0_dec2", _p(128, 4, 256, 5, 7, 3, 2, "parallel", gth=1, n_enc=0, n_dec=2)),
    # ---- swizzled 32 x 32 tiles with and without phantom row tiles (16x16, one memory frame, parallel: 1024 rows at D = 128)
    ("m1024_d128", _p(128, 4, 256, 16, 16, 3, 1, "parallel", n_dec=1)),
    # ---- the workload: 24 x 36 maps, two memory frames, 10 objects, cls + bbreg (5184 rows)
    ("deployed", _p(256, 8, 2048, 24, 36, 10, 2, "parallel", gth=1, n_enc=6, n_dec=6)),
])
DEPLOYED = "deployed"
PARAM_SEED, INPUT_SEED = 9100, 9200           # + 10 x the case's position in the table (+ the sequence, + 1000 x the object)


def absent_objects(T):
    """The objects whose labels and boxes are zero: a middle one whenever there are at least three."""
    return (T // 2,) if T >= 3 else ()


def expand(text):
    out, stack = [], []
    for tok in text.split():
        if tok.endswith("*["):
            stack.append((int(tok[:-2]), len(out)))
        elif tok == "]":
            n, at = stack.pop()
            out += out[at:] * (n - 1)
        else:
            assert tok in R or tok in RT, tok
            out.append(tok)
    assert not stack
    return tuple(out)


def compress(names):
    """The greedy inverse of expand(): immediate repetitions of a block of up to 12 names become N*[ block ]."""
    names, out, i = list(names), [], 0
    while i < len(names):
        best = (1, 1)
        for w in range(1, 13):
            n = 1
            while names[i + n * w:i + (n + 1) * w] == names[i:i + w]:
                n += 1
            if n > 1 and n * w > best[0] * best[1]:
                best = (n, w)
        n, w = best
        out.append(names[i] if n == 1 else f"{n}*[ " + compress(names[i:i + w]) + " ]")
        i += n * w
    return " ".join(out)


# The pinned routes, in launch order: written by `python tests/tamos_f64.py` from pt_tamos_predict_routes, then read against the launcher.
ROUTES_TEXT = {
    "base_t3": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "base_t1": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "base_t10": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD 2*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "base_t11": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD 2*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "base_t16": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD 2*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "mask9_gth0": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD GEMM_T32 GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN256 2*[ GEMM_T32_SWZ ] 2*[ LN256 GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN256 GEMM_T32 TAMOS_XATTN256 TAMOS_XMERGE GEMM_T32 LN256 2*[ GEMM_T32 ] ] 2*[ LN256 ] TO_NCHW",
    "mask9_gth1": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD GEMM_T32 GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN256 2*[ GEMM_T32_SWZ ] 2*[ LN256 GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN256 GEMM_T32 TAMOS_XATTN256 TAMOS_XMERGE GEMM_T32 LN256 2*[ GEMM_T32 ] ] 2*[ LN256 ] TO_NCHW",
    "mask9_gth2": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD GEMM_T32 GEMM_T32_SWZ ATTN32 GEMM_T32_SWZ LN256 2*[ GEMM_T32_SWZ ] 2*[ LN256 GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN256 GEMM_T32 TAMOS_XATTN256 TAMOS_XMERGE GEMM_T32 LN256 2*[ GEMM_T32 ] ] 2*[ LN256 ] TO_NCHW",
    "keys1444": "TAMOS_TOKENS TAMOS_BOX1 2*[ GEMM_T32_SWZ_PAD ] GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ_PAD LN256 GEMM_T32_SWZ_PAD GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 2*[ GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN256 GEMM_T32 TAMOS_XATTN256 TAMOS_XMERGE GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 ] LN256 TO_NCHW",
    "head16_keys1452": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32_SWZ_PAD ] ATTN16 GEMM_T32_SWZ_PAD LN128 2*[ GEMM_T32_SWZ_PAD ] 2*[ LN128 GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] ] 2*[ LN128 ] TO_NCHW",
    "head64_seq3": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ 2*[ GEMM_T32 ] ATTN64 2*[ 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN_GENERIC GEMM_T32 TAMOS_XATTN512 TAMOS_XMERGE ] GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] 2*[ LN_GENERIC ] TO_NCHW",
    "d384_t3": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] ATTN64 2*[ 2*[ GEMM_T32 LN_GENERIC GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN_GENERIC GEMM_T32 TAMOS_XATTN384 TAMOS_XMERGE ] GEMM_T32 LN_GENERIC 2*[ GEMM_T32 ] 2*[ LN_GENERIC ] TO_NCHW",
    "seq1": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] ATTN32 2*[ 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE ] GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "seq2": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] ATTN32 2*[ 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE ] GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "seq8": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ_PAD 2*[ GEMM_T32 ] ATTN32 2*[ 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE ] GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "dec1": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] 2*[ ATTN32 2*[ GEMM_T32 LN128 GEMM_T32 ] ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "enc0_dec2": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE 2*[ GEMM_T32 LN128 GEMM_T32 ] TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "m1024_d128": "TAMOS_TOKENS TAMOS_BOX1 3*[ GEMM_T32_SWZ ] ATTN32 GEMM_T32_SWZ LN128 2*[ GEMM_T32_SWZ ] LN128 GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN128 GEMM_T32 TAMOS_XATTN128 TAMOS_XMERGE GEMM_T32 LN128 2*[ GEMM_T32 ] 2*[ LN128 ] TO_NCHW",
    "deployed": "TAMOS_TOKENS TAMOS_BOX1 GEMM_T32_SWZ GEMM_T32_SWZ_PAD 6*[ GEMM_PS2_WIDE ATTN32 GEMM_T32_SWZ_PAD LN256 GEMM_PS4_WIDE GEMM_PS4_SPLITK_WIDE LN256_SPLIT4 ] 6*[ GEMM_T32 TAMOS_SELF_ATTN GEMM_T32 LN256 GEMM_T32 TAMOS_XATTN256 TAMOS_XMERGE GEMM_T32 LN256 2*[ GEMM_T32 ] LN256 ] LN256 TO_NCHW",
}

ROUTES = {name: expand(text) for name, text in ROUTES_TEXT.items()}

# max |fp32 restatement - float64 restatement| per output group (tests/tamos_f64.py), as measured on the CPU the table was written on
REF_ERR = {
    "base_t3": {"predictor": 1.070e-06, "scores": 8.487e-06},
    "base_t1": {"predictor": 8.431e-07, "scores": 9.241e-06},
    "base_t10": {"predictor": 1.124e-06, "scores": 1.220e-05},
    "base_t11": {"predictor": 9.862e-07, "scores": 1.336e-05},
    "base_t16": {"predictor": 1.102e-06, "scores": 1.176e-05},
    "mask9_gth0": {"predictor": 9.390e-07, "scores": 2.371e-05},
    "mask9_gth1": {"predictor": 2.234e-06, "scores": 2.332e-05},
    "mask9_gth2": {"predictor": 1.054e-06, "scores": 2.058e-05},
    "keys1444": {"predictor": 1.403e-06, "scores": 3.277e-05},
    "head16_keys1452": {"predictor": 1.476e-06, "scores": 1.622e-05},
    "head64_seq3": {"predictor": 1.714e-06, "scores": 4.008e-05},
    "d384_t3": {"predictor": 1.285e-06, "scores": 1.879e-05},
    "seq1": {"predictor": 6.323e-07, "scores": 1.177e-05},
    "seq2": {"predictor": 7.596e-07, "scores": 9.453e-06},
    "seq8": {"predictor": 1.118e-06, "scores": 1.332e-05},
    "dec1": {"predictor": 8.835e-07, "scores": 1.057e-05},
    "enc0_dec2": {"predictor": 1.089e-06, "scores": 2.712e-06},
    "m1024_d128": {"predictor": 8.437e-07, "scores": 1.019e-05},
    "deployed": {"predictor": 3.071e-06, "scores": 5.519e-05},
}


def dims(cfg):
    return _lib.TompDims(cfg["D"], cfg["nhead"], cfg["ff"], cfg["n_enc"], cfg["n_dec"], cfg["H"], cfg["W"], cfg["feature_sz"])


def route_name(v):
    if 0 < v < len(R):
        return R[v]
    assert _lib.TAMOS_ROUTE_BASE <= v < _lib.TAMOS_ROUTE_BASE + len(RT), v
    return RT[v - _lib.TAMOS_ROUTE_BASE]


def query(L, d, T, n_train, n_seq, parallel):
    """(status, route names) of pt_tamos_predict_routes"""
    cap = _lib.PT_TAMOS_MAX_ROUTES
    out = (ctypes.c_int * cap)(*([-1] * cap))
    n = ctypes.c_int(-1)
    rc = L.pt_tamos_predict_routes(ctypes.byref(d), T, n_train, n_seq, parallel, out, cap, ctypes.byref(n))
    if rc != 0:
        assert n.value == 0 and not any(out), (rc, n.value)
        return rc, ()
    assert 0 < n.value <= cap and not any(out[n.value:])
    return rc, tuple(route_name(v) for v in out[:n.value])


def case_routes(L, name):
    cfg = CASES[name]
    return query(L, dims(cfg), cfg["T"], cfg["n_train"], cfg["n_seq"], int(cfg["mode"] == "parallel"))


# ------------------------------------------------------------------------------------------------------------------
# parameters, inputs, modules
# ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def case(name):
    """(cfg, parameters {'fp.' / 'cls.' + reference key: fp32 numpy}, (train (n,ns,D,H,W), test (1,ns,D,H,W), label (n,ns,T,H,W),
    ltrb (n,ns,T,4,H,W)) fp32 numpy), generated once per session and read-only."""
    if name not in _CACHE:
        cfg = CASES[name]
        k = list(CASES).index(name)
        D, T = cfg["D"], cfg["T"]
        params = {q: v for q, v in synth.tomp_params(PARAM_SEED + 10 * k, cfg).items()
                  if not q.startswith("reg.") and q != "fp.query_embed_test.weight"}
        rng = np.random.default_rng(PARAM_SEED + 10 * k + 5)
        E = rng.standard_normal((T, D))
        params["fp.query_embed_fg.weight"] = (E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)   # unit rows, as orthogonal_ leaves them
        seqs = []
        for s in range(cfg["n_seq"]):
            objs = [synth.tomp_inputs(INPUT_SEED + 10 * k + s + 1000 * o, cfg) for o in range(T)]
            lab = np.stack([o[2][:, 0] for o in objs], axis=1)[:, None]               # (n, 1, T, H, W)
            ltrb = np.stack([o[3][:, 0] for o in objs], axis=1)[:, None]              # (n, 1, T, 4, H, W)
            for a in absent_objects(T):
                lab[:, :, a] = 0
                ltrb[:, :, a] = 0
            seqs.append((objs[0][0], objs[0][1], lab, ltrb))
        inputs = tuple(np.ascontiguousarray(np.concatenate([s[i] for s in seqs], axis=1)) for i in range(4))
        for v in list(params.values()) + list(inputs):
            v.setflags(write=False)
        _CACHE[name] = (cfg, params, inputs)
    return _CACHE[name]


def state_dict(params, prefix):
    sd = {k[len(prefix):]: torch.from_numpy(v.copy()) for k, v in params.items() if k.startswith(prefix)}
    if prefix == "fp.":
        for idx in (1, 4):
            sd[f"box_encoding.{idx}.num_batches_tracked"] = torch.tensor(0)
    return sd


def build_modules(cfg, params, device):
    """The mirrored GOTFilterPredictor and LinearFilterClassifier carrying the seeded parameters, loaded with strict=True under the
    reference's key names."""
    from pytracking_amd import tamos as TA
    from pytracking_amd import transformer as TM
    tr = TM.Transformer(d_model=cfg["D"], nhead=cfg["nhead"], num_encoder_layers=cfg["n_enc"], num_decoder_layers=cfg["n_dec"],
                        dim_feedforward=cfg["ff"])
    pred = TA.GOTFilterPredictor(tr, feature_sz=cfg["feature_sz"], num_tokens=cfg["T"], label_enc="gaussian", box_enc="ltrb_token")
    cls = TM.LinearFilterClassifier(num_channels=cfg["D"])
    pred.load_state_dict(state_dict(params, "fp."), strict=True)
    cls.load_state_dict(state_dict(params, "cls."), strict=True)
    return pred.to(device).eval(), cls.to(device).eval()
