"""Cases, seeded inputs and float64 numpy restatements of ECO's Fourier-domain per-frame path (pytracking_amd/eco.py, eco.hip), shared by
tests/test_eco_cpu.py, tests/test_gpu_eco.py and tools/make_golden_eco.py.  Inputs come from pytracking_amd.synth by seed; the goldens
(tests/golden/eco_*.npz) hold only outputs of the unmodified reference run on a two-function torch.rfft / torch.irfft shim (the installed
torch has neither), which tests/test_eco_cpu.py checks against a float64 dense DFT.  Reads nothing outside the repository.  Test
infrastructure only.

The restatements are dense: every transform is a product with explicit matrices of exp(+-2 pi i k n / N), k n kept as integers.
`track_frames(ops, state, feats)` is ECO.track's per-frame sequence (eco.py:181-241) written once over an `ops` namespace, so that the same
loop runs on float64 numpy (NumpyOps), on pytracking_amd.eco's torch forms and on the kernels (tests/test_gpu_eco.py)."""
import itertools
import math
import os
from collections import OrderedDict

import numpy as np

import f64_bound
from pytracking_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = f64_bound.ULP            # one fp32 ulp of 1, under the name tools/make_golden_eco_init.py and tests/test_eco_cpu.py use
SAMPLE_ENTRIES = 256          # entries of a large output a golden keeps (seeded positions)


def series_sizes(H, W):
    return H + (H + 1) % 2, W // 2 + 1


# ---------------------------------------------------------------------------------------------------------------------------
# case tables

SAMPLE_SIZES = ((4, 4), (5, 5), (6, 9), (1, 1), (15, 15), (60, 60))
SAMPLE_CHANNELS = ((3, 2), (96, 16), (256, 64), (5, None))            # (Cin, c); None: no projection
SAMPLE_CASES = OrderedDict()
for _i, ((_H, _W), (_Cin, _c), _S, _sh) in enumerate(itertools.product(SAMPLE_SIZES, SAMPLE_CHANNELS, (1, 5), (False, True))):
    SAMPLE_CASES[f"{_H}x{_W}_{_Cin}to{_c or 'same'}_S{_S}_{'shift' if _sh else 'plain'}"] = dict(
        seed=7000 + _i, H=_H, W=_W, Cin=_Cin, c=_c, S=_S, shift=(0.31, -0.17) if _sh else None)

APPLY_CASES = OrderedDict((
    ("5x3_c2_S1", dict(seed=7200, S=1, c=2, Hf=5, Wh=3)),
    ("7x4_c4_S1", dict(seed=7201, S=1, c=4, Hf=7, Wh=4)),
    ("15x8_c64_S5", dict(seed=7202, S=5, c=64, Hf=15, Wh=8)),
    ("61x31_c16_S5", dict(seed=7203, S=5, c=16, Hf=61, Wh=31)),
))

# blocks: (Hf, Wh) of every block in the tracker's order; grid (Oh, Ow); weights None = fusion 'sum'
LOC_CASES = OrderedDict((
    ("one_61_equal_S1", dict(seed=7300, S=1, blocks=((61, 31),), grid=(61, 61), weights=None)),
    ("one_61_240_S5_w", dict(seed=7310, S=5, blocks=((61, 31),), grid=(240, 240), weights=(0.7,))),
    ("two_61_15_240_S5", dict(seed=7320, S=5, blocks=((61, 31), (15, 8)), grid=(240, 240), weights=None)),
    ("two_61_15_240_S5_w", dict(seed=7330, S=5, blocks=((61, 31), (15, 8)), grid=(240, 240), weights=(0.4, 0.6))),
    ("two_15_61_odd_S1_w", dict(seed=7340, S=1, blocks=((15, 8), (61, 31)), grid=(63, 65), weights=(0.6, 0.4))),
    ("two_9_7_equal_S5", dict(seed=7350, S=5, blocks=((9, 5), (7, 4)), grid=(9, 9), weights=None)),
    ("two_9_7_even_S1_w", dict(seed=7360, S=1, blocks=((9, 5), (7, 4)), grid=(12, 10), weights=(0.4, 0.6))),
    ("two_7_9_odd_S5", dict(seed=7370, S=5, blocks=((7, 4), (9, 5)), grid=(11, 13), weights=None)),
    ("one_7_9x13_S1", dict(seed=7380, S=1, blocks=((7, 4),), grid=(9, 13), weights=None)),
    ("one_7_9x13_S5_w", dict(seed=7390, S=5, blocks=((7, 4),), grid=(9, 13), weights=(1.3,))),
))

INSERT_CASES = OrderedDict()
for _i, (_ind, _sh) in enumerate(itertools.product((0, 3, 6), (None, (0.23, -0.41)))):
    INSERT_CASES[f"9x5_c4_n7_slot{_ind}_{'shift' if _sh else 'plain'}"] = dict(seed=7400 + _i, Hf=9, Wh=5, c=4, n=7, ind=_ind, shift=_sh)
INSERT_CASES["61x31_c16_n200_slot199_shift"] = dict(seed=7410, Hf=61, Wh=31, c=16, n=200, ind=199, shift=(-0.05, 0.6))
INSERT_CASES["15x8_c64_n200_slot100_plain"] = dict(seed=7411, Hf=15, Wh=8, c=64, n=200, ind=100, shift=None)


# ---------------------------------------------------------------------------------------------------------------------------
# inputs (float32 numpy, from seeds)

def sample_inputs(case):
    c = SAMPLE_CASES[case] if isinstance(case, str) else case
    x = synth.eco_features(c["seed"], c["S"], c["Cin"], c["H"], c["W"])
    P = None if c["c"] is None else synth.eco_projection(c["seed"] + 1, c["Cin"], c["c"])
    return x, P, synth.eco_window(c["H"], c["W"]), synth.eco_interp(c["seed"] + 2, c["H"], c["W"]), c["shift"]


def apply_inputs(case):
    c = APPLY_CASES[case]
    return synth.eco_series(c["seed"], 1, c["c"], c["Hf"], c["Wh"]), synth.eco_series(c["seed"] + 1, c["S"], c["c"], c["Hf"], c["Wh"])


_LOC_SEEDS = {}


def loc_inputs(case):
    """The blocks' responses of a localisation case.  The seed moves on until, in float64, every scale's maximum exceeds every other value of
    its map by 1e-4 of the score range (the whole map, not only outside the peak's neighbourhood: arg-max positions are compared exactly
    and no case needs an exclusion)."""
    c = LOC_CASES[case]
    seed = _LOC_SEEDS.get(case, c["seed"])
    while True:
        sfs = [synth.eco_series(seed + 10 * b, c["S"], 1, hf, wh, decay=0.15) for b, (hf, wh) in enumerate(c["blocks"])]
        scores = localize_np(sfs, c["weights"], c["grid"])[0]
        flat = np.sort(scores.reshape(c["S"], -1), axis=1)
        if ((flat[:, -1] - flat[:, -2]) >= 1e-4 * (scores.max() - scores.min())).all():
            _LOC_SEEDS[case] = seed
            return sfs
        seed += 1
        assert seed < c["seed"] + 10, case


def insert_inputs(case):
    c = INSERT_CASES[case]
    mem = synth.eco_series(c["seed"], c["n"], c["c"], c["Hf"], c["Wh"]).transpose(2, 3, 0, 1, 4).copy()      # (Hf, Wh, n, c, 2)
    return mem, synth.eco_series(c["seed"] + 1, 1, c["c"], c["Hf"], c["Wh"])


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatements

def to_c(a):
    a = np.asarray(a, dtype=np.float64)
    return a[..., 0] + 1j * a[..., 1]


def to_r(z):
    return np.stack((z.real, z.imag), -1)


def phases(k, n, N, sign):
    """exp(sign 2 pi i k n / N) as a (len(k), len(n)) matrix, k n reduced mod N in integers."""
    kn = np.mod(np.outer(np.asarray(k, dtype=np.int64), np.asarray(n, dtype=np.int64)), N)
    return np.exp(sign * 2j * math.pi * kn / N)


def centred(Hf):
    return np.arange(Hf) - (Hf - 1) // 2


def cfft2_np(y):
    """(..., H, W) real -> (..., Hf, Wh) complex: the centred one-sided dense DFT."""
    H, W = y.shape[-2:]
    Hf, Wh = series_sizes(H, W)
    rows = np.asarray(y, dtype=np.float64) @ phases(np.arange(Wh), np.arange(W), W, -1).T            # (..., H, Wh)
    return phases(centred(Hf), np.arange(H), H, -1) @ rows


def shift_np(z, shift):
    """complex (..., Hf, Wh)"""
    Hf, Wh = z.shape[-2:]
    return z * np.exp(1j * shift[0] * centred(Hf))[:, None] * np.exp(1j * shift[1] * np.arange(Wh))[None, :]


def sample_np(x, P, window, interp, shift=None):
    y = np.asarray(x, dtype=np.float64)
    if P is not None:
        y = np.einsum("sihw,ik->skhw", y, np.asarray(P, dtype=np.float64))
    if window is not None:
        y = y * np.asarray(window, dtype=np.float64).reshape(y.shape[-2:])
    z = cfft2_np(y)
    if interp is not None:
        z = z * to_c(interp[0]).reshape(-1)[:, None] * to_c(interp[1]).reshape(-1)[None, :]
    if shift is not None:
        z = shift_np(z, shift)
    return to_r(z)


def apply_filter_np(hf, xf):
    return to_r((to_c(hf) * to_c(xf)).sum(1, keepdims=True))


def sum_blocks_np(sfs, weights):
    order = sorted(range(len(sfs)), key=lambda b: sfs[b].shape[2], reverse=True)
    total = None
    for b in order:
        e = to_c(sfs[b]) * (1.0 if weights is None else float(weights[b]))
        if total is None:
            total = e.copy()
            mid = (total.shape[2] - 1) // 2
        else:
            top = mid - (e.shape[2] - 1) // 2
            total[:, :, top:top + e.shape[2], :e.shape[3]] += e
    return total


def max2d_np(scores):
    """dcf.max2d on (..., H, W): the column of the largest column maximum, then that column's first maximal row."""
    col_max, col_row = scores.max(-2), scores.argmax(-2)
    col = col_max.argmax(-1)
    row = np.take_along_axis(col_row, col[..., None], -1)[..., 0]
    return np.take_along_axis(col_max, col[..., None], -1)[..., 0], np.stack((row, col), -1)


def localize_np(sfs, weights, grid):
    """-> scores (S, 1, Oh, Ow), max_val (S, 1), argmax (S, 1, 2): the real part of the half-spectrum series, kx = 0 once, kx > 0 twice."""
    a = sum_blocks_np(sfs, weights)
    Hf, Wh = a.shape[2:]
    Oh, Ow = int(grid[0]), int(grid[1])
    ex = phases(np.arange(Ow), np.arange(Wh), Ow, +1) * np.where(np.arange(Wh) == 0, 1.0, 2.0)[None, :]
    scores = np.einsum("yr,scrk,xk->scyx", phases(np.arange(Oh), centred(Hf), Oh, +1), a, ex).real
    mv, am = max2d_np(scores)
    return scores, mv, am


def insert_np(mem, xf, ind, shift=None):
    z = to_c(xf)
    if shift is not None and (shift[0] != 0 or shift[1] != 0):
        z = shift_np(z, shift)
    out = np.array(mem, dtype=np.float64)
    out[:, :, ind] = to_r(z)[0].transpose(1, 2, 0, 3)
    return out


def sample_positions(seed, size):
    """The flat positions of a large output that its golden keeps."""
    return np.arange(size) if size <= 4 * SAMPLE_ENTRIES else np.sort(np.random.default_rng(seed).choice(size, SAMPLE_ENTRIES, replace=False))


# ---------------------------------------------------------------------------------------------------------------------------
# the per-frame loop

class NumpyOps:
    """The float64 side of track_frames."""
    @staticmethod
    def sample_transform(x, P, window, interp):
        return sample_np(x, P, window, interp)

    @staticmethod
    def apply_filter(hf, xf):
        return apply_filter_np(hf, xf)

    @staticmethod
    def localize(sfs, weights, grid):
        return localize_np(sfs, weights, grid)

    @staticmethod
    def insert(mem, xf, ind, shift):
        mem[...] = insert_np(mem, xf, ind, shift)

    @staticmethod
    def host(a):
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def train(state, new_xf, sw, num_iter, forget):
        """FilterOptim.run on the loop's state; the CG state (p, rho, r_prev) is carried in state["cg"]."""
        opt = FilterOptimNp(state["filter"], state["memory"], [sw] * len(new_xf), state["yf"], state["regs"], state["energy"], state["lrs"],
                            state["reg_energy"], forget=forget)
        if state["cg"] is not None:
            opt.p, opt.rho, opt.r_prev = state["cg"]
        opt.run(num_iter, new_xf)
        state["cg"] = (opt.p, opt.rho, opt.r_prev)
        for f, x, e, en in zip(state["filter"], opt.x, state["energy"], opt.energy):
            f[...] = to_r(x)
            e[...] = en


LOOP = dict(seed=7503, frames=12, train_skipping=5, cg_iter=3, forget=0.9 ** 75, S=3, n=6, blocks=((8, 8, 6, 3), (4, 4, 10, 4)), scale_step=1.02, upsample=2, support=32.0,
            weights=(0.4, 0.6), lr=0.1, image=(120.0, 160.0), pos=(60.0, 80.0), target=(20.0, 24.0))        # block: (H, W, Cin, c)


def loop_state(xp=np.asarray):
    """The post-initialisation state of the closed loop: per block a filter, a projection, window, interpolation factors and a sample memory
    with n slots of which two are filled; `xp` converts every float32 array (numpy: identity; the device tests pass an uploader)."""
    c = LOOP
    st = dict(filter=[], proj=[], window=[], interp=[], memory=[], weights=[], yf=[], regs=[], energy=[], reg_energy=[], lrs=[], cg=None)
    for b, (H, W, Cin, cc) in enumerate(c["blocks"]):
        Hf, Wh = series_sizes(H, W)
        P, win, interp = synth.eco_projection(c["seed"] + b, Cin, cc), synth.eco_window(H, W), synth.eco_interp(c["seed"] + 10 + b, H, W)
        target = sample_np(synth.eco_features(c["seed"] + 50 + b, 1, Cin, H, W), P, win, interp)
        hf = to_r(np.conj(to_c(target)) / (np.abs(to_c(target)) ** 2).sum(1, keepdims=True).clip(1e-3))             # a matched filter
        mem = np.zeros((Hf, Wh, c["n"], cc, 2), dtype=np.float32)
        mem[:, :, 0] = target[0].transpose(1, 2, 0, 3)
        st["filter"].append(xp(hf.astype(np.float32)))
        st["proj"].append(xp(P))
        st["window"].append(xp(win))
        st["interp"].append((xp(interp[0]), xp(interp[1])))
        st["memory"].append(xp(mem))
        ky, kx = np.arange(Hf) - (Hf - 1) // 2, np.arange(Wh)
        st["yf"].append(xp((np.exp(-0.5 * (ky[:, None] / 1.5) ** 2 - 0.5 * (kx[None, :] / 1.5) ** 2) / (Hf * W)).astype(np.float32).reshape(1, 1, Hf, Wh)))
        st["regs"].append(xp(fu_reg(3, 3, b)))
        st["reg_energy"].append(float((fu_reg(3, 3, b).astype(np.float64) ** 2).sum()))
        st["energy"].append(xp(np.ascontiguousarray((target ** 2).sum(-1)).astype(np.float32)))
        st["lrs"].append(c["lr"])
    return st


def loop_features(frame):
    """The S scales' feature maps of every block at `frame`: the target's own maps plus frame noise, rolled by a frame-dependent offset."""
    c = LOOP
    out = []
    for b, (H, W, Cin, cc) in enumerate(c["blocks"]):
        base = synth.eco_features(c["seed"] + 50 + b, 1, Cin, H, W)[0]
        noise = synth.eco_features(c["seed"] + 100 + 10 * frame + b, c["S"], Cin, H, W)
        x = np.stack([np.roll(base, (frame % 3 - 1, frame % 2), axis=(1, 2))] * c["S"])
        gain = (1.0 - 0.05 * np.abs(np.arange(c["S"]) - frame % c["S"])).astype(np.float32)[:, None, None, None]
        out.append((x * gain + np.float32(0.3) * noise).astype(np.float32))
    return out


def track_frames(ops, state, feats, xp=np.asarray):
    """ECO.track (eco.py:181-241) for `len(feats)` frames, the filter trained on every frame with frame_num % train_skipping == 1 (frame
    numbers start at 2, as after initialize()).  Host state (position, scale, sample weights) is float64 everywhere.  Returns per frame
    the box, max_score, scale_ind and the memory slot written, then the final memories and filters."""
    c = LOOP
    S = c["S"]
    scale_factors = c["scale_step"] ** (np.arange(S) - (S - 1) // 2)
    support = np.array([c["support"]] * 2)
    out_sz = c["upsample"] * support
    pos, target_scale = np.array(c["pos"], dtype=np.float64), 1.0
    base_target, image = np.array(c["target"]), np.array(c["image"])
    sw = np.zeros(c["n"])
    sw[0] = 1.0
    prev_ind, stored = None, 1
    log = []
    for frame_num, x in enumerate(feats, start=2):
        sample_pos = np.round(pos)
        sample_scales = target_scale * scale_factors
        xf = [ops.sample_transform(xp(xe), P, w, i) for xe, P, w, i in zip(x, state["proj"], state["window"], state["interp"])]
        sf = [ops.apply_filter(h, e) for h, e in zip(state["filter"], xf)]
        scores, max_val, argmax = ops.localize(sf, c["weights"], out_sz)
        max_val, argmax = ops.host(max_val).reshape(S), ops.host(argmax).reshape(S, 2)
        scale_ind = int(np.argmax(max_val))
        disp = (argmax[scale_ind] + out_sz / 2) % out_sz - out_sz / 2
        tv = disp * (support / out_sz) * target_scale * scale_factors[scale_ind]
        target_scale = float(np.clip(target_scale * scale_factors[scale_ind], (10 / base_target).max(), (image / base_target).min()))
        tsz = base_target * target_scale
        pos = np.maximum(np.minimum(sample_pos + tv, image + 0.3 * tsz), -0.3 * tsz)
        shift = 2 * math.pi * (pos - sample_pos) / (sample_scales[scale_ind] * support)
        # update_sample_weights (eco.py:346-370), one learning rate
        if stored == 0:
            ind = 0
        else:
            ind = int(np.argmin(sw))
            if prev_ind is None:
                sw /= 1 - c["lr"]
                sw[ind] = c["lr"]
            else:
                sw[ind] = sw[prev_ind] / (1 - c["lr"])
        sw /= sw.sum()
        prev_ind, stored = ind, stored + 1
        train_xf = []
        for mem, e in zip(state["memory"], xf):
            ops.insert(mem, e[scale_ind:scale_ind + 1], ind, (float(shift[0]), float(shift[1])))
            train_xf.append(mem[:, :, ind:ind + 1].transpose(2, 3, 0, 1, 4) if isinstance(mem, np.ndarray) else mem[:, :, ind:ind + 1].permute(2, 3, 0, 1, 4))
        if frame_num % c["train_skipping"] == 1:
            ops.train(state, train_xf, sw, c["cg_iter"], c["forget"])
        box = np.concatenate((pos[::-1] - (tsz[::-1] - 1) / 2, tsz[::-1]))
        log.append(dict(box=box, max_score=float(max_val[scale_ind]), scale_ind=scale_ind, slot=ind, trained=frame_num % c["train_skipping"] == 1))
    return log, [ops.host(m) for m in state["memory"]] + [ops.host(f) for f in state["filter"]]


# ---------------------------------------------------------------------------------------------------------------------------
# filter update (FilterOptim.run): float64 restatement and cases

def ip_np(a, b):
    """fourier.inner_prod_fs of complex (1, c, Hf, Wh) arrays: 2 <a, b> - <a[.., 0], b[.., 0]> over real and imaginary parts."""
    d = a.real * b.real + a.imag * b.imag
    return 2.0 * d.sum() - d[..., 0].sum()


def reg_np(v, reg):
    """The regulariser of FilterOptim.A (optim.py:177-198) on complex v (1, c, Hf, Wh) with the real filter reg (Rh, Rw)."""
    _, c, Hf, Wh = v.shape
    Rh, Rw = reg.shape
    pad1, pad2 = min(Rh - 1, Hf - 1), min(Rw - 1, 2 * Wh - 2)
    ext = np.concatenate((np.conj(v[..., 1:pad2 + 1][..., ::-1, ::-1]), v), -1) if pad2 > 0 else v

    def corr(x, ph, pw):
        x = np.pad(x, ((0, 0), (0, 0), (ph, ph), (pw, pw)))
        oh, ow = x.shape[2] - Rh + 1, x.shape[3] - Rw + 1
        out = np.zeros(x.shape[:2] + (oh, ow), dtype=x.dtype)
        for a in range(Rh):
            for b in range(Rw):
                out += reg[a, b] * x[:, :, a:a + oh, b:b + ow]
        return out
    first = corr(ext, pad1, pad2)
    return corr(first[..., min(pad2, Wh - 1):], 0, 0)


class FilterOptimNp:
    """FilterOptim (optim.py:121-208) with run_CG (optimization.py:72-163) in float64; per block complex arrays, scalars per block, joint exit."""

    def __init__(self, filters, samples, weights, yf, regs, energy, lrs, reg_energy, fr=False, std_alpha=True, forget=0.0, dp=0.3, rp=0.15,
                 single=False):
        cd, fd = (np.complex64, np.float32) if single else (np.complex128, np.float64)       # single: what fp32 arithmetic costs on the case
        self.x = [to_c(f).astype(cd) for f in filters]
        self.S = [to_c(s).astype(cd) for s in samples]           # (Hf, Wh, n, c)
        self.w = [np.asarray(w, dtype=fd) for w in weights]
        self.yf = [np.asarray(y, dtype=fd).reshape(y.shape[-2:]) for y in yf]
        self.reg = [np.asarray(r, dtype=fd).reshape(r.shape[-2:]) for r in regs]
        self.energy = [np.asarray(e, dtype=fd) for e in energy]
        self.lrs, self.reg_energy, self.fr, self.std_alpha, self.forget, self.dp, self.rp = lrs, reg_energy, fr, std_alpha, forget, dp, rp
        self.p, self.rho, self.r_prev = None, [1.0] * len(filters), None

    def A(self, v):
        out = []
        for S, w, reg, e in zip(self.S, self.w, self.reg, v):
            sh = (S @ e[0].transpose(1, 2, 0)[..., None])[..., 0] * w                       # (Hf, Wh, n)
            out.append((sh[..., None, :] @ np.conj(S))[..., 0, :].transpose(2, 0, 1)[None] + reg_np(e, reg))
        return out

    def run(self, num_iter, new_xf=None):
        if num_iter == 0:
            return
        nb = len(self.x)
        if new_xf is not None:
            self.energy = [(1 - lr) * e + lr * (np.abs(to_c(nx)) ** 2).astype(e.dtype) for lr, e, nx in zip(self.lrs, self.energy, new_xf)]
        b = [y[None, None] * np.conj((w[None, None, None, :] @ S)[..., 0, :].transpose(2, 0, 1))[None] for y, w, S in zip(self.yf, self.w, self.S)]
        dM = [(1 - self.rp) * (self.dp * e + (1 - self.dp) * e.mean(1, keepdims=True)) + self.rp * re for e, re in zip(self.energy, self.reg_energy)]
        if self.forget == 0:
            self.p, self.rho, self.r_prev = None, [1.0] * nb, None
        elif self.p is not None:
            self.rho = [r / self.forget for r in self.rho]
        r = [bb - q for bb, q in zip(b, self.A(self.x))]
        for ii in range(num_iter):
            z = [rr / d for rr, d in zip(r, dM)]
            rho1, self.rho = self.rho, [ip_np(rr, zz) for rr, zz in zip(r, z)]
            if any(v == 0 for v in self.rho):
                return
            if self.p is None:
                self.p = [zz.copy() for zz in z]
            else:
                beta = [(n / o if self.fr else (n - ip_np(rp, zz)) / o) for n, o, rp, zz in zip(self.rho, rho1, self.r_prev or z, z)]
                self.p = [zz + pp * max(bt, 0.0) for zz, pp, bt in zip(z, self.p, beta)]
            q = self.A(self.p)
            pq = [ip_np(pp, qq) for pp, qq in zip(self.p, q)]
            alpha = [(rh if self.std_alpha else ip_np(pp, rr)) / v for rh, pp, rr, v in zip(self.rho, self.p, r, pq)]
            if not self.fr:
                self.r_prev = [rr.copy() for rr in r]
            self.x = [xx + pp * al for xx, pp, al in zip(self.x, self.p, alpha)]
            if ii < num_iter - 1:
                r = [rr - qq * al for rr, qq, al in zip(r, q, alpha)]


def fu_reg(Rh, Rw, seed=0):
    """A real regularisation filter (1, 1, Rh, Rw), symmetric as get_reg_filter's, with a dominant centre."""
    g = np.random.default_rng(7900 + seed).uniform(0.002, 0.01, (Rh, Rw))
    g = 0.5 * (g + g[::-1, ::-1])
    g[Rh // 2, Rw // 2] = 0.05
    return g.astype(np.float32).reshape(1, 1, Rh, Rw)


# name: blocks ((Hf, Wh, c, n, (Rh, Rw)), ...), iterations per call, options
FU_CASES = OrderedDict((
    ("5x3_c2_n3", dict(seed=7600, blocks=((5, 3, 2, 3, (3, 3)),), iters=(3,))),
    # Wh = 2: the reference's complex.is_complex takes the real (1, 1, Hf, 2) label function for a complex tensor and raises: no golden
    ("3x2_c4_n1", dict(seed=7610, blocks=((3, 2, 4, 1, (1, 1)),), iters=(2,), no_ref=True)),
    ("two_blocks", dict(seed=7620, blocks=((9, 5, 4, 6, (5, 5)), (7, 4, 8, 6, (3, 3))), iters=(4,))),
    ("n200_7_weights", dict(seed=7630, blocks=((9, 5, 4, 200, (5, 5)),), iters=(3,), nonzero=7)),
    ("reg_1x1", dict(seed=7640, blocks=((9, 5, 4, 6, (1, 1)),), iters=(3,))),
    ("reg_7x1", dict(seed=7650, blocks=((9, 5, 4, 6, (7, 1)),), iters=(3,))),
    ("fletcher_reeves", dict(seed=7660, blocks=((9, 5, 4, 6, (5, 5)),), iters=(4,), fr=True)),
    ("alpha_from_residual", dict(seed=7670, blocks=((9, 5, 4, 6, (5, 5)),), iters=(4,), std_alpha=False)),
    ("forget_three_calls", dict(seed=7680, blocks=((9, 5, 4, 6, (5, 5)), (7, 4, 8, 6, (3, 3))), iters=(3, 3, 3), forget=0.975 ** 75)),
    ("forget_three_calls_fr", dict(seed=7685, blocks=((9, 5, 4, 6, (5, 5)),), iters=(3, 3, 3), forget=0.975 ** 75, fr=True)),
    ("one_iteration", dict(seed=7690, blocks=((9, 5, 4, 6, (5, 5)),), iters=(1,))),
    ("zero_iterations", dict(seed=7700, blocks=((9, 5, 4, 6, (5, 5)),), iters=(0,))),
    ("no_new_sample", dict(seed=7710, blocks=((9, 5, 4, 6, (5, 5)),), iters=(3,), new_xf=False)),
    ("deployed_deep", dict(seed=7720, blocks=((15, 8, 64, 200, (3, 3)),), iters=(5, 5), forget=0.9925 ** 75)),
    ("deployed_shallow", dict(seed=7730, blocks=((61, 31, 16, 200, (5, 5)),), iters=(5, 5), forget=0.975 ** 75)),
))


def fu_inputs(case):
    """Per block: filter, sample memory built by pushing spatially correlated features through the sample transform (a real spectrum's decay),
    sample weights, label function, reg filter, sample energy; per call and block a new sample.  float32 numpy."""
    c = FU_CASES[case] if isinstance(case, str) else case
    out = dict(filters=[], samples=[], weights=[], yf=[], regs=[], energy=[], new_xf=[[] for _ in c["iters"]], lrs=[], reg_energy=[])
    for b, (Hf, Wh, cc, n, (Rh, Rw)) in enumerate(c["blocks"]):
        seed = c["seed"] + 100 * b
        H, W = Hf, 2 * Wh - 1
        interp = synth.eco_interp(seed + 1, H, W)
        xf = sample_np(synth.eco_features(seed, n + len(c["iters"]), cc, H, W), None, synth.eco_window(H, W), interp).astype(np.float32) * np.float32(8.0)
        out["samples"].append(np.ascontiguousarray(xf[:n].transpose(2, 3, 0, 1, 4)))
        for k in range(len(c["iters"])):
            out["new_xf"][k].append(np.ascontiguousarray(xf[n + k:n + k + 1]))
        w = synth.decay_weights(n, 0.05).astype(np.float32)
        if c.get("nonzero"):
            w[:n - c["nonzero"]] = 0
            w /= w.sum()
        out["weights"].append(w)
        ky, kx = np.arange(Hf) - (Hf - 1) // 2, np.arange(Wh)
        out["yf"].append((np.exp(-0.5 * (ky[:, None] / 1.5) ** 2 - 0.5 * (kx[None, :] / 1.5) ** 2) / (Hf * W)).astype(np.float32).reshape(1, 1, Hf, Wh))
        out["regs"].append(fu_reg(Rh, Rw, b))
        out["energy"].append(((xf[:n] ** 2).sum(-1).mean(0, keepdims=True)).astype(np.float32))
        out["filters"].append(synth.eco_series(seed + 2, 1, cc, Hf, Wh) * np.float32(0.01))
        out["lrs"].append(0.025 if b == 0 else 0.0075)
        out["reg_energy"].append(float((out["regs"][-1].astype(np.float64) ** 2).sum()))
    return out


def fu_run_np(case, single=False):
    """The float64 (or, `single`, fp32) run of a case -> per call the filters after it, and the final energies."""
    c = FU_CASES[case]
    d = fu_inputs(case)
    opt = FilterOptimNp(d["filters"], d["samples"], d["weights"], d["yf"], d["regs"], d["energy"], d["lrs"], d["reg_energy"], c.get("fr", False),
                        c.get("std_alpha", True), c.get("forget", 0.0), single=single)
    outs = []
    for k, it in enumerate(c["iters"]):
        opt.run(it, d["new_xf"][k] if c.get("new_xf", True) else None)
        outs.append([to_r(x) for x in opt.x])
    return outs, opt.energy
