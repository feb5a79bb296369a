"""Edge shapes of the three fused modules that no golden reaches, shared by tests/test_fused_edge_cases_cpu.py and
tests/test_gpu_fused_f64.py.  State and inputs come from the seeded generators of pytracking_amd.synth; the expected value is the float64
stand-in of tests/fused_f64.py, so none of these cases has (or needs) a golden and none is part of synth.*_CASES.  Every case names the
code edge it is there for; tests/test_fused_edge_cases_cpu.py asserts that each is covered and lands on the route it claims.  Test
infrastructure only."""
from collections import OrderedDict

import torch

import fused_f64 as F64
import iou_feat_cases as IC
import label_enc_cases as LC
import lwl_decoder_cases as DC
from pytracking_amd import synth

BANDED, GEMM = "banded", "gemm"

# name: dict(n, mdim, ic, use_bn, levels = ((layer, fc, H, W), ...) deepest first, image, scores) as synth.LWL_DECODER_CASES
DECODER = OrderedDict((
    # mdim 64: fc 48 leaves one wave of k_dec_conv1 without a chunk, fc 80 gives wave 0 two; 32 channels into k_dec_conv_out; odd ratios
    ("mdim64", dict(n=1, mdim=64, ic=16, use_bn=True, levels=(("layer4", 48, 2, 3), ("layer3", 80, 4, 5), ("layer2", 48, 7, 9), ("layer1", 16, 13, 17)),
                    image=(45, 61), scores=(3, 4))),
    # mdim 96: oc + ic is no multiple of 64 on any level, 48 channels into k_dec_conv_out; layer1 and the Upsampler on the GEMM route with padded weights (k_iou_padw)
    ("mdim96", dict(n=2, mdim=96, ic=16, use_bn=True, levels=(("layer4", 32, 1, 22), ("layer3", 48, 2, 43), ("layer2", 16, 3, 86), ("layer1", 16, 5, 172)),
                    image=(19, 700), scores=(2, 45))),
    # n = 8 (DEC_MAX_N); layer1's 32-channel 1x1 convolutions reach k_dec_conv1<4> with a ragged last tile (2021 positions), layer2's stay just below the switch
    ("n8_wide1x1", dict(n=8, mdim=32, ic=16, use_bn=True, levels=(("layer4", 32, 5, 7), ("layer3", 32, 11, 13), ("layer2", 16, 29, 31), ("layer1", 16, 43, 47)),
                        image=(100, 115), scores=(11, 13))),
    # three levels at n = 8 without BatchNorm; every 3x3 runs the plan of the same sample alone, so the per-sample check is bit for bit
    ("three_n8", dict(n=8, mdim=32, ic=16, use_bn=False, levels=(("layer3", 32, 3, 5), ("layer2", 16, 6, 9), ("layer1", 16, 11, 17)),
                      image=(40, 63), scores=(4, 6))),
))
# the route of every 3x3 convolution of a level / of the Upsampler's first convolution that a case claims
DECODER_ROUTES = {
    "mdim64": {"layer4": BANDED, "layer3": BANDED, "layer2": BANDED, "layer1": BANDED, "up": BANDED},
    "mdim96": {"layer4": BANDED, "layer3": BANDED, "layer2": BANDED, "layer1": GEMM, "up": GEMM},
    "n8_wide1x1": {"layer4": BANDED, "layer3": BANDED, "layer2": BANDED, "layer1": BANDED, "up": BANDED},
    "three_n8": {"layer3": BANDED, "layer2": BANDED, "layer1": BANDED, "up": BANDED},
}

# name: (n, H, W, layer_dims, use_bn) as synth.LABEL_ENC_CASES.  Limits of label_enc.hip: dims % 16 == 0 and <= 64; a stem workgroup makes
# 4 x 32 pooled outputs from 128 mask columns; the output is ceil(H / 16) x ceil(W / 16).
LABEL_ENC = OrderedDict((
    ("m1x1", (1, 1, 1, synth.LABEL_ENC_DIMS, False)),         # one pixel: every tap but the centre is padding at every stage
    ("m1x17", (1, 1, 17, synth.LABEL_ENC_DIMS, False)),       # one row: no vertical neighbour anywhere, two output columns
    ("m17x1", (1, 17, 1, synth.LABEL_ENC_DIMS, False)),       # one column, two output rows
    ("h15", (2, 15, 40, synth.LABEL_ENC_DIMS, False)),        # one below the /16 boundary: one output row, the last stem row odd
    ("h16", (2, 16, 40, synth.LABEL_ENC_DIMS, True)),         # exactly /16, with BatchNorm
    ("h17", (2, 17, 40, synth.LABEL_ENC_DIMS, False)),        # one past: a second output row made from one mask row
    ("w127", (1, 9, 127, synth.LABEL_ENC_DIMS, False)),       # one column short of a stem tile's 128 mask columns
    ("w128", (1, 9, 128, synth.LABEL_ENC_DIMS, False)),       # exactly one stem tile
    ("w129", (1, 9, 129, synth.LABEL_ENC_DIMS, True)),        # one column into the second stem tile
    ("n33", (33, 20, 37, synth.LABEL_ENC_DIMS, False)),       # one mask more than the tracker stores: grid z and the per-image strides
    ("c16", (2, 21, 35, (16, 16, 16, 16), False)),            # the smallest channel counts: one channel tile everywhere but the fused layers
    ("c64", (2, 21, 35, (64, 64, 64, 64), True)),             # LE_MAX_C everywhere: eight channel tiles in the fused conv1 | downsample
    ("c48", (2, 21, 35, (16, 48, 64, 48), True)),             # 48: three channel tiles (T = 1), six in the fused layers (T = 2)
))

# name: (n, (Cin3, Cmid3, Cout3, H3, W3), (Cin4, Cmid4, Cout4, H4, W4)) as synth.IOU_FEAT_CASES
IOU_ROW_LIMIT = 170                                           # widest row of the banded route (asserted with pt_mf_corr_tm_plan)
IOU_FEAT = OrderedDict((
    # n = 8 (IOU_MAX_N), Cin = 192 in both towers (three 64-channel steps: % 64 but not % 128), Cmid != Cout
    ("n8_c192", (8, (192, 32, 48, 5, 7), (192, 48, 16, 3, 4))),
    # a 1x1 map next to a row exactly at the banded route's limit
    ("row_limit", (1, (192, 32, 48, 1, 1), (64, 16, 32, 2, IOU_ROW_LIMIT))),
    # a 1x1 map next to a row one past it: the GEMM route with Cin = 192 and a padded second layer (Cmid 48)
    ("row_past", (1, (64, 32, 16, 1, 1), (192, 48, 32, 2, IOU_ROW_LIMIT + 1))),
))
IOU_ROUTES = {"n8_c192": (BANDED, BANDED), "row_limit": (BANDED, BANDED), "row_past": (BANDED, GEMM)}      # (tower 3, tower 4)

CASES = {"iou_feat": tuple(IOU_FEAT), "label_enc": tuple(LABEL_ENC), "lwl_decoder": tuple(DECODER)}
PER_SAMPLE = (("iou_feat", "n8_c192"), ("label_enc", "n33"), ("lwl_decoder", "n8_wide1x1"), ("lwl_decoder", "three_n8"))
STATE_SEED, INPUT_SEED = {"iou_feat": 8100, "label_enc": 8300, "lwl_decoder": 8500}, {"iou_feat": 8200, "label_enc": 8400, "lwl_decoder": 8600}
_CACHE = {}


def case(kind, name):
    """(stand-in module in fp32 on the CPU, CPU arguments as fused_f64.standin takes them), generated once per session."""
    if (kind, name) not in _CACHE:
        k = CASES[kind].index(name)
        sseed, iseed = STATE_SEED[kind] + k, INPUT_SEED[kind] + k
        if kind == "iou_feat":
            n, t3, t4 = IOU_FEAT[name]
            net = IC.Towers(t3, t4)
            net.load_state_dict(IC.state_tensors(synth.iou_feat_state(sseed, t3[0], t4[0], t3[1], t3[2], t4[1], t4[2])))
            f3, f4 = synth.iou_feat_inputs(iseed, n, t3[0], t3[3], t3[4], t4[0], t4[3], t4[4])
            args = dict(feats=(torch.from_numpy(f3), torch.from_numpy(f4)))
        elif kind == "label_enc":
            n, H, W, dims, use_bn = LABEL_ENC[name]
            net = LC.ResidualDS16SW(dims, use_bn)
            net.load_state_dict(LC.state_tensors(synth.label_enc_state(sseed, dims, use_bn)))
            args = dict(masks=torch.from_numpy(synth.label_enc_masks(iseed, n, H, W))[:, None])
        else:
            c = DECODER[name]
            net = DC.Decoder(c["ic"], c["mdim"], OrderedDict((L, fc) for L, fc, _, _ in c["levels"]), c["use_bn"])
            net.load_state_dict(DC.state_tensors(synth.lwl_decoder_state(sseed, c["mdim"], c["ic"], c["use_bn"], c["levels"])))
            s, feats = synth.lwl_decoder_inputs(iseed, c["n"], c["ic"], c["levels"], c["scores"])
            args = dict(scores=torch.from_numpy(s), feats={L: torch.from_numpy(v) for L, v in feats.items()}, image=tuple(c["image"]),
                        names=DC.level_names(c))
        _CACHE[(kind, name)] = (net.eval(), args)
    return _CACHE[(kind, name)]


def anchor(kind, name):
    net, args = case(kind, name)
    return F64.anchor(kind, ("edge", name), net, args)


def samples(kind, name):
    """Number of samples of a case."""
    return {"iou_feat": lambda: IOU_FEAT[name][0], "label_enc": lambda: LABEL_ENC[name][0], "lwl_decoder": lambda: DECODER[name]["n"]}[kind]()


def sample(kind, args, k):
    """The arguments of sample k alone (n = 1)."""
    if kind == "iou_feat":
        return dict(feats=tuple(f[k:k + 1] for f in args["feats"]))
    if kind == "label_enc":
        return dict(masks=args["masks"][k:k + 1])
    return dict(args, scores=args["scores"][k:k + 1], feats={L: v[k:k + 1] for L, v in args["feats"].items()})


# ---- the 3x3 convolutions of a case, for the plan query (pt_mf_corr_tm_plan) ------------------------------------------------------------
def conv3_shapes(kind, name):
    """OrderedDict {stage: [(Cout, Cin, H, W), ...]} of the 3x3 convolutions that choose between the banded and the GEMM route: the levels
    and the Upsampler's first convolution of a decoder case (lwl_decoder.hip, dec_plan), the two towers of an IoU case."""
    out = OrderedDict()
    if kind == "iou_feat":
        _, t3, t4 = IOU_FEAT[name]
        for tag, t in (("tower3", t3), ("tower4", t4)):
            out[tag] = [(t[1], t[0], t[3], t[4]), (t[2], t[1], t[3], t[4])]
        return out
    c = DECODER[name]
    for L, _, H, W in c["levels"]:
        oc = DC.OC[L] * c["mdim"]
        nc = oc + c["ic"]
        out[L] = [(nc, nc, H, W), (nc, nc, H, W), (oc, nc, H, W)] + [(oc, oc, H, W)] * 4
    _, _, H, W = c["levels"][-1]
    out["up"] = [(c["mdim"] // 2, c["mdim"], 2 * H, 2 * W)]
    return out


def plans(lib, kind, name, n=None):
    """{stage: [plan, ...]} with plan = (ks, br, npg, nb, last band, Wp) of the banded route or GEMM, for n samples (default: the case's)."""
    import corr_tm_cases as TC
    n = samples(kind, name) if n is None else n
    out = OrderedDict()
    for stage, convs in conv3_shapes(kind, name).items():
        out[stage] = []
        for cout, cin, H, W in convs:
            rc, p = TC.query(lib, n, cout, cin, H, W)
            out[stage].append(tuple(p) if rc == 0 else GEMM)
    return out


def routes_coincide(lib, kind, name):
    """Does every 3x3 convolution of the case run the same banded plan with all its samples as with one sample alone?  Only then is the
    order of every sum the same and a sample's output the same bits either way: the channel splits (ks) are summed in another order when
    they differ, and the GEMM route tiles n * H * W tokens.  The label encoder has no split accumulation and no route (label_enc.hip: the
    tile choice moves outputs between workgroups, never terms between sums), and k_dec_conv1<1> / <4> add the same chunks in the same
    order, so neither enters."""
    if kind == "label_enc":
        return True
    a, b = plans(lib, kind, name), plans(lib, kind, name, 1)
    return a == b and all(p != GEMM for ps in a.values() for p in ps)


def wide_1x1(HW, cout, n):
    """dec_conv1's switch (lwl_decoder.hip): k_dec_conv1<4> when ceil(HW / 64) * (Cout / 16) * n >= 512."""
    return ((HW + 63) // 64) * (cout // 16) * n >= 512
