"""ECO's Fourier-domain per-frame path (pytracking/tracker/eco/eco.py:181-245) on gfx950 (eco.hip):

  sample_transform(x, proj, window, interp, shift)   project_sample + preprocess_sample (+ shift_fs)             -> pt_eco_sample_f32
  shift_fs(a, shift)                                 fourier.shift_fs                                            -> pt_eco_shift_f32
  apply_filter(hf, xf)                               ECO.apply_filter                                            -> pt_eco_apply_filter_f32
  localize(sfs, weights, grid)                       sum_fs + sample_fs + dcf.max2d of ECO.localize_target       -> pt_eco_localize_f32
  insert(samples, xf, ind, shift)                    shift_fs + ECO.update_memory's slot store                   -> pt_eco_insert_f32
  filter_update(filters, samples, ...)               FilterOptim.run (preconditioned CG, all blocks)             -> pt_eco_filter_update_f32

and the first-frame joint optimisation of filter and projection matrix (eco.py:152-158) (eco_init.hip):

  joint_init(filters, projections, samples, ...)     GaussNewtonCG.run on FactorizedConvProblem (all blocks)     -> pt_eco_joint_init_f32

`torch.rfft` / `torch.irfft`, which fourier.py:24,31 and dcf.py:134,139 call, do not exist in the installed torch, so the stock ECO cannot
run at all.  `cfft2`, `cifft2` and `get_reg_filter` below are written on `torch.fft` from the documented behaviour of the removed functions
(one-sided, unnormalised forward transform over the last two dimensions, complex numbers as a trailing dimension of 2; normalised inverse
with `signal_sizes`); install(eco=True) binds them in place of the reference's.  They work on any device and dtype.

Every operation has a plain-torch form (`*_torch`, any device, any floating dtype) that states what the kernel computes; the tests run it in
float64 and in fp32.  The `tracker_*` functions take the reference's ECO object and its TensorLists; `covered_*` say whether a call runs on
the kernels, install() hands every other call to the reference.  `gauss_newton_cg` builds the class install(eco_init=True) binds under
the name eco.py:9 imported: the reference's GaussNewtonCG whose `run` takes the kernels for ECO's FactorizedConvProblem on the device.
"""
import ctypes
import math

import torch

from . import _lib
from ._packs import dev_f32 as _dev_f32, no_grad_needed as _no_grad_needed, require_device as _require_device
from .filter import _ptr, _stream, device_guarded, workspace


def series_sizes(H, W):
    """(Hf, Wh) of the centred half spectrum of an (H, W) map: always an odd number of rows."""
    return H + (H + 1) % 2, W // 2 + 1


# ---------------------------------------------------------------------------------------------------------------------------
# the Fourier tools on torch.fft (any device, any floating dtype)

def cfft2(a):
    """fourier.cfft2: the one-sided 2-D transform of the last two dimensions of (..., H, W), rows reordered to the frequencies
    -(Hf - 1) / 2 .. (Hf - 1) / 2 (for even H the Nyquist row at both ends) -> (..., Hf, Wh, 2)."""
    H = a.shape[-2]
    Hf = series_sizes(H, a.shape[-1])[0]
    spec = torch.view_as_real(torch.fft.rfftn(a, dim=(-2, -1)))
    rows = (torch.arange(Hf, device=a.device) - (Hf - 1) // 2) % H
    return spec.index_select(spec.dim() - 3, rows)


def cifft2(a, signal_sizes=None):
    """fourier.cifft2: the inverse of cfft2 for a centred half spectrum (..., Hf, Wh, 2); without `signal_sizes` the result has
    2 (Wh - 1) columns, as the removed torch.irfft returned."""
    rows_dim = a.dim() - 3
    spec = torch.roll(a, -((a.shape[rows_dim] - 1) // 2), rows_dim).contiguous()
    sizes = None if signal_sizes is None else [int(v) for v in signal_sizes]
    return torch.fft.irfftn(torch.view_as_complex(spec), s=sizes, dim=(-2, -1))


def get_reg_filter(sz, target_sz, params):
    """dcf.get_reg_filter: the spatial regulariser of CCOT / ECO as a small real filter in the Fourier domain, (1, 1, Rh, Rw)."""
    if not params.use_reg_window:
        return params.reg_window_min * torch.ones(1, 1, 1, 1)
    if getattr(params, 'reg_window_square', False):
        target_sz = target_sz.prod().sqrt() * torch.ones(2)
    half = 0.5 * target_sz

    def axis(n):
        neg, pos = torch.arange(-int((n - 1) / 2), 0, dtype=torch.float32), torch.arange(0, int(n / 2 + 1), dtype=torch.float32)
        return torch.cat([neg, pos]) if getattr(params, 'reg_window_centered', True) else torch.cat([pos, neg])

    rows, cols = axis(sz[0]).view(1, 1, -1, 1), axis(sz[1]).view(1, 1, 1, -1)
    power, floor = params.reg_window_power, params.reg_window_min
    window = (params.reg_window_edge - floor) * (torch.abs(rows / half[0]) ** power + torch.abs(cols / half[1]) ** power) + floor
    spec = torch.view_as_real(torch.fft.rfftn(window, dim=(-2, -1))) / sz.prod()
    mag = spec.pow(2).sum(-1).sqrt()
    spec[mag < params.reg_sparsity_threshold * mag.max(), :] = 0
    # the sparse window's minimum moves away from reg_window_min: the DC coefficient takes the difference
    sparse = torch.fft.irfftn(torch.view_as_complex(spec.contiguous()), s=sz.long().tolist(), dim=(-2, -1))
    spec[0, 0, 0, 0, 0] += floor - sz.prod() * sparse.min()
    H = spec.shape[2]
    Hf = series_sizes(H, 1)[0]
    real = spec[..., 0].index_select(2, (torch.arange(Hf) - (Hf - 1) // 2) % H)
    last = real.nonzero().max(dim=0)[0]
    mid = (Hf - 1) // 2
    real = real[..., 2 * mid - last[-2].item():last[-2].item() + 1, :last[-1].item() + 1]
    if real.shape[-1] > 1:
        real = torch.cat([real[..., 1:].flip((2, 3)), real], -1)
    return real


# ---------------------------------------------------------------------------------------------------------------------------
# plain-torch forms of the five operations (complex numbers as a trailing dimension of 2)

def _cmul(a, b):
    return torch.stack((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), -1)


def _as_complex_factor(t, rows, n):
    """An interpolation factor of `n` frequencies as (1, 1, n, 1, 2) / (1, 1, 1, n, 2): real factors (no centring) get a zero imaginary part."""
    t = torch.stack((t.reshape(-1), torch.zeros_like(t.reshape(-1))), -1) if t.numel() == n else t.reshape(-1, 2)
    return t.reshape(1, 1, -1, 1, 2) if rows else t.reshape(1, 1, 1, -1, 2)


def shift_fs_torch(a, shift):
    s0, s1 = float(shift[0]), float(shift[1])
    if s0 == 0 and s1 == 0:
        return a
    Hf, Wh = a.shape[2], a.shape[3]
    ky = torch.arange(-((Hf - 1) // 2), Hf // 2 + 1, dtype=a.dtype, device=a.device).view(1, 1, -1, 1)
    kx = torch.arange(0, Wh, dtype=a.dtype, device=a.device).view(1, 1, 1, -1)
    ey = torch.stack((torch.cos(s0 * ky), torch.sin(s0 * ky)), -1)
    ex = torch.stack((torch.cos(s1 * kx), torch.sin(s1 * kx)), -1)
    return _cmul(_cmul(a, ey), ex)


def sample_transform_torch(x, proj, window, interp, shift=None):
    if proj is not None:
        x = torch.matmul(x.permute(2, 3, 0, 1), proj).permute(2, 3, 0, 1)
    if window is not None:
        x = x * window.reshape(1, 1, *x.shape[-2:])
    xf = cfft2(x)
    if interp is not None:
        xf = _cmul(_cmul(xf, _as_complex_factor(interp[0], True, xf.shape[2])), _as_complex_factor(interp[1], False, xf.shape[3]))
    return xf if shift is None else shift_fs_torch(xf, shift)


def apply_filter_torch(hf, xf):
    return _cmul(hf, xf).sum(1, keepdim=True)


def sum_blocks_torch(sfs, weights=None):
    """fourier.sum_fs of the (weighted) blocks, the largest first."""
    total = None
    for b, e in enumerate(sfs):
        e = e if weights is None else weights[b] * e
        if total is None:
            total = e.clone()
            mid = (total.shape[-3] - 1) // 2
        else:
            top = mid - (e.shape[-3] - 1) // 2
            total[..., top:top + e.shape[-3], :e.shape[-2], :] += e
    return total


def localize_torch(sfs, weights, grid):
    """-> scores (S, 1, Oh, Ow), max_val (S, 1), argmax (S, 1, 2): the real part of the half-spectrum series on the grid (include/pt_hot.h)
    by zero padding and the inverse real transform, then dcf.max2d's arg-max."""
    order = sorted(range(len(sfs)), key=lambda b: sfs[b].shape[2], reverse=True)          # stable, as sum_fs sorts
    a = sum_blocks_torch([sfs[b] for b in order], None if weights is None else [weights[b] for b in order])
    Hf, Wh = a.shape[2], a.shape[3]
    Oh, Ow = int(grid[0]), int(grid[1])
    top = (Oh - Hf) // 2
    pad = torch.nn.functional.pad(a, (0, 0, 0, Ow // 2 + 1 - Wh, top, Oh - Hf - top))
    scores = float(Oh * Ow) * cifft2(pad, signal_sizes=(Oh, Ow))
    col_max, col_row = scores.max(dim=-2)
    max_val, col = col_max.max(dim=-1)
    row = col_row.gather(-1, col.unsqueeze(-1)).squeeze(-1)
    return scores, max_val, torch.stack((row, col), -1)


def insert_torch(samples, xf, ind, shift=None):
    if shift is not None:
        xf = shift_fs_torch(xf, shift)
    samples[:, :, ind:ind + 1, :, :] = xf.permute(2, 3, 0, 1, 4)
    return samples


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def covered_sample(x, proj, window, interp) -> bool:
    if not _dev_f32(x, 4) or min(x.shape) < 1 or max(x.shape[-2:]) > _lib.PT_ECO_MAX_FEAT:
        return False
    H, W = x.shape[-2:]
    Hf, Wh = series_sizes(H, W)
    if proj is not None and not (_dev_f32(proj, 2) and proj.shape[0] == x.shape[1] and proj.shape[1] >= 1):
        return False
    if window is not None and not (_dev_f32(window) and window.numel() == H * W):
        return False
    if interp is not None:
        if not (isinstance(interp, (tuple, list)) and len(interp) == 2 and _dev_f32(interp[0]) and _dev_f32(interp[1])):
            return False
        if interp[0].numel() not in (Hf, 2 * Hf) or interp[1].numel() not in (Wh, 2 * Wh):
            return False
    return _no_grad_needed(x, proj, window, *(interp or ()))


def _shift_args(shift):
    if shift is None:
        return 0, 0.0, 0.0
    s0, s1 = float(shift[0]), float(shift[1])
    return int(s0 != 0 or s1 != 0), s0, s1


@device_guarded
def sample_transform(x, proj, window, interp, shift=None):
    """x (S, Cin, H, W), proj (Cin, c) or None, window (H, W)-shaped or None, interp = (interp_y, interp_x) or None, shift = two angles or
    None -> xf (S, c, Hf, Wh, 2)."""
    _require_device(x, proj, window)
    if not covered_sample(x, proj, window, interp):
        raise NotImplementedError(f"sample transform: device fp32 (S, Cin, H, W) with H, W <= {_lib.PT_ECO_MAX_FEAT}, no grad")
    S, Cin, H, W = x.shape
    c = Cin if proj is None else proj.shape[1]
    Hf, Wh = series_sizes(H, W)
    xc = x.contiguous()
    pc = proj.contiguous() if proj is not None else None
    wc = window.contiguous() if window is not None else None
    iy = ix = None
    if interp is not None:
        iy, ix = _as_complex_factor(interp[0], True, Hf).contiguous(), _as_complex_factor(interp[1], False, Wh).contiguous()
    out = torch.empty((S, c, Hf, Wh, 2), dtype=torch.float32, device=x.device)
    null = ctypes.c_void_p(None)
    has, s0, s1 = _shift_args(shift)
    rc = _lib.lib().pt_eco_sample_f32(_ptr(xc), _ptr(pc) if pc is not None else null, _ptr(wc) if wc is not None else null,
                                      _ptr(iy) if iy is not None else null, _ptr(ix) if ix is not None else null, has, s0, s1, _ptr(out),
                                      S, Cin, c, H, W, _stream())
    _lib.check(rc, "pt_eco_sample_f32")
    return out


def covered_series(a) -> bool:
    return _dev_f32(a, 5) and a.shape[-1] == 2 and min(a.shape) >= 1 and a.shape[2] % 2 == 1 and a.numel() <= 1 << 30 and _no_grad_needed(a)


@device_guarded
def shift_fs(a, shift):
    _require_device(a)
    if not covered_series(a):
        raise NotImplementedError("shift_fs: device fp32 (S, c, Hf, Wh, 2) with odd Hf, no grad")
    has, s0, s1 = _shift_args(shift)
    if not has:
        return a
    ac = a.contiguous()
    out = torch.empty_like(ac)
    S, c, Hf, Wh, _ = ac.shape
    _lib.check(_lib.lib().pt_eco_shift_f32(_ptr(ac), s0, s1, _ptr(out), S, c, Hf, Wh, _stream()), "pt_eco_shift_f32")
    return out


def covered_apply_filter(hf, xf) -> bool:
    return (covered_series(hf) and covered_series(xf) and hf.shape[0] == 1 and hf.shape[1:] == xf.shape[1:] and hf.device == xf.device
            and hf.shape[2] * hf.shape[3] <= 1 << 24)


@device_guarded
def apply_filter(hf, xf):
    """hf (1, c, Hf, Wh, 2), xf (S, c, Hf, Wh, 2) -> sf (S, 1, Hf, Wh, 2)."""
    _require_device(hf, xf)
    if not covered_apply_filter(hf, xf):
        raise NotImplementedError("apply_filter: device fp32 hf (1, c, Hf, Wh, 2) and xf (S, c, Hf, Wh, 2), no grad")
    S, c, Hf, Wh, _ = xf.shape
    h, x = hf.contiguous(), xf.contiguous()
    sf = torch.empty((S, 1, Hf, Wh, 2), dtype=torch.float32, device=xf.device)
    _lib.check(_lib.lib().pt_eco_apply_filter_f32(_ptr(h), _ptr(x), _ptr(sf), S, c, Hf, Wh, _stream()), "pt_eco_apply_filter_f32")
    return sf


def covered_localize(sfs, grid) -> bool:
    sfs = list(sfs)
    if not 1 <= len(sfs) <= _lib.PT_ECO_MAX_BLOCKS or not all(covered_series(e) and e.shape[1] == 1 for e in sfs):
        return False
    big = max(sfs, key=lambda e: e.shape[2])
    if any(e.shape[0] != big.shape[0] or e.shape[3] > big.shape[3] or e.device != big.device for e in sfs):
        return False
    Oh, Ow = int(grid[0]), int(grid[1])
    if Oh != grid[0] or Ow != grid[1] or Oh < big.shape[2] or Ow < 2 * big.shape[3] - 1:
        return False
    return _lib.lib().pt_eco_localize_ws_bytes(big.shape[0], big.shape[3], Oh, Ow) > 0


@device_guarded
def localize(sfs, weights, grid):
    """sfs: the blocks' responses (S, 1, Hf_b, Wh_b, 2); weights: one float per block or None; grid (Oh, Ow) -> scores (S, 1, Oh, Ow),
    max_val (S, 1), argmax (S, 1, 2) int64.  Definition in include/pt_hot.h."""
    sfs = list(sfs)
    _require_device(*sfs)
    if not covered_localize(sfs, grid):
        raise NotImplementedError(f"localize: <= {_lib.PT_ECO_MAX_BLOCKS} device fp32 blocks (S, 1, Hf, Wh, 2), Wh <= 64, a grid of at least "
                                  f"the series' size and at most {_lib.PT_ECO_MAX_GRID} points a side, no grad")
    order = sorted(range(len(sfs)), key=lambda b: sfs[b].shape[2], reverse=True)          # stable, as sum_fs sorts
    blocks = [sfs[b].contiguous() for b in order]
    nb, S, Oh, Ow = len(blocks), blocks[0].shape[0], int(grid[0]), int(grid[1])
    dev = blocks[0].device
    ptrs = (ctypes.c_void_p * nb)(*[e.data_ptr() for e in blocks])
    hfs = (ctypes.c_int * nb)(*[e.shape[2] for e in blocks])
    whs = (ctypes.c_int * nb)(*[e.shape[3] for e in blocks])
    wts = None if weights is None else (ctypes.c_float * nb)(*[float(weights[b]) for b in order])
    scores = torch.empty((S, 1, Oh, Ow), dtype=torch.float32, device=dev)
    max_val = torch.empty((S, 1), dtype=torch.float32, device=dev)
    argmax = torch.empty((S, 1, 2), dtype=torch.int64, device=dev)
    L = _lib.lib()
    ws = workspace(L.pt_eco_localize_ws_bytes(S, blocks[0].shape[3], Oh, Ow), dev)
    rc = L.pt_eco_localize_f32(ptrs, hfs, whs, wts, nb, S, Oh, Ow, _ptr(scores), _ptr(max_val), _ptr(argmax), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_eco_localize_f32")
    return scores, max_val, argmax


def covered_insert(samples, xf, ind) -> bool:
    return (_dev_f32(samples, 5) and samples.is_contiguous() and covered_series(xf) and xf.shape[0] == 1 and samples.shape[-1] == 2
            and samples.device == xf.device and tuple(samples.shape[:2]) == tuple(xf.shape[2:4]) and samples.shape[3] == xf.shape[1]
            and isinstance(ind, int) and 0 <= ind < samples.shape[2] and samples.numel() <= 1 << 31 and _no_grad_needed(samples))


@device_guarded
def insert(samples, xf, ind, shift=None):
    """Store xf (1, c, Hf, Wh, 2), shifted by `shift` when given, into slot `ind` of samples (Hf, Wh, n, c, 2), in place."""
    _require_device(samples, xf)
    if not covered_insert(samples, xf, ind):
        raise NotImplementedError("insert: contiguous device fp32 samples (Hf, Wh, n, c, 2) and xf (1, c, Hf, Wh, 2), 0 <= ind < n, no grad")
    Hf, Wh, n, c, _ = samples.shape
    x = xf.contiguous()
    has, s0, s1 = _shift_args(shift)
    _lib.check(_lib.lib().pt_eco_insert_f32(_ptr(x), has, s0, s1, _ptr(samples), c, Hf, Wh, n, ind, _stream()), "pt_eco_insert_f32")
    return samples


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's call boundary (install(eco=True)): `tracker` is the unmodified ECO object, lists are its TensorLists

def covered_cfft2(a) -> bool:
    return covered_sample(a, None, None, None)


def cfft2_device(a):
    return sample_transform(a, None, None, None)


def _blocks_on_device(tracker, *names):
    return all(all(_dev_f32(t) for t in (e if isinstance(e, (tuple, list)) else (e,))) for name in names for e in getattr(tracker, name))


def covered_preprocess_sample(tracker, x) -> bool:
    if getattr(tracker.params, "debug", 0) >= 3 or len(x) != len(tracker.window):
        return False
    return all(covered_sample(xe, None, w, i) for xe, w, i in zip(x, tracker.window, tracker.interp_fs))


def tracker_preprocess_sample(tracker, x):
    """ECO.preprocess_sample (eco.py:297-300); like the reference it leaves `x` multiplied by the window."""
    out = type(x)([sample_transform(xe, None, w, i) for xe, w, i in zip(x, tracker.window, tracker.interp_fs)])
    x *= tracker.window
    return out


def covered_extract_fourier_sample(tracker, im, pos, scales, sz) -> bool:
    return getattr(tracker.params, "debug", 0) < 3 and _blocks_on_device(tracker, "window", "interp_fs", "projection_matrix")


def tracker_extract_fourier_sample(tracker, im, pos, scales, sz):
    """ECO.extract_fourier_sample (eco.py:293-295): projection, window, transform and interpolation factors of a block in one launch."""
    x = tracker.extract_sample(im, pos, scales, sz)
    args = list(zip(x, tracker.projection_matrix, tracker.window, tracker.interp_fs))
    if len(x) != len(tracker.window) or not all(covered_sample(*a) for a in args):
        return tracker.preprocess_sample(tracker.project_sample(x))           # features of another kind: the bound methods decide
    return type(x)([sample_transform(*a) for a in args])


def covered_tracker_apply_filter(tracker, sample_xf) -> bool:
    return (getattr(tracker.params, "debug", 0) < 3 and len(sample_xf) == len(tracker.filter)
            and all(covered_apply_filter(h, x) for h, x in zip(tracker.filter, sample_xf)))


def tracker_apply_filter(tracker, sample_xf):
    return type(sample_xf)([apply_filter(h, x) for h, x in zip(tracker.filter, sample_xf)])


def _grid_of(tracker):
    return [float(v) for v in tracker.output_sz]


def covered_localize_target(tracker, sf) -> bool:
    if tracker.params.score_fusion_strategy not in ("sum", "weightedsum") or getattr(tracker.params, "debug", 0) >= 3:
        return False
    grid = _grid_of(tracker)
    if not covered_localize(sf, grid):
        return False
    big = max(sf, key=lambda e: e.shape[2])
    return (int(grid[0]), int(grid[1])) != (big.shape[2], 2 * big.shape[3] - 1)      # the equal grid: see include/pt_hot.h


def tracker_localize_target(tracker, sf):
    """ECO.localize_target (eco.py:247-287) for 'sum' and 'weightedsum': the series sum, its evaluation and the arg-max on the device;
    the reference's own host arithmetic on the S arg-max positions follows."""
    weights = None
    if tracker.params.score_fusion_strategy == "weightedsum":
        weights = [float(w) for w in tracker.fparams.attribute('translation_weight')]
    scores, max_score, max_disp = localize(sf, weights, _grid_of(tracker))
    _, scale_ind = torch.max(max_score.cpu(), dim=0)      # a host index: it selects from host tensors (scale factors, displacements)
    max_disp = max_disp.float().cpu()
    disp = (max_disp + tracker.output_sz / 2) % tracker.output_sz - tracker.output_sz / 2
    translation_vec = disp[scale_ind, ...].view(-1) * (tracker.img_support_sz / tracker.output_sz) * tracker.target_scale
    translation_vec *= tracker.params.scale_factors[scale_ind]
    return translation_vec, scale_ind, scores


def covered_shift_fs(a, shift) -> bool:
    return isinstance(a, torch.Tensor) and a.dim() == 5 and covered_series(a)


def covered_update_memory(tracker, sample_xf) -> bool:
    return (getattr(tracker.params, "debug", 0) < 3 and len(sample_xf) == len(tracker.training_samples)
            and all(covered_insert(m, x, 0) for m, x in zip(tracker.training_samples, sample_xf)))


def tracker_update_memory(tracker, sample_xf):
    """ECO.update_memory (eco.py:339-343): the sample weights stay on the host as in the reference, the slot store is one launch per block."""
    replace_ind = tracker.update_sample_weights()
    for mem, xf, ind in zip(tracker.training_samples, sample_xf, replace_ind):
        insert(mem, xf, int(ind))


def shift_angles(pos, sample_pos, scale, img_support_sz):
    """The two angles ECO.track hands to shift_fs (eco.py:226)."""
    return [2 * math.pi * float(p - q) / (float(scale) * float(s)) for p, q, s in zip(pos, sample_pos, img_support_sz)]


# ---------------------------------------------------------------------------------------------------------------------------
# filter update (FilterOptim.run)

def new_cg_state(filters):
    """The carried CG state of pt_eco_filter_update_f32 for the given filters: per block p, r_prev (the filter's shape) and state = [rho, p valid]."""
    return [dict(p=torch.zeros_like(f), r_prev=torch.zeros_like(f), state=torch.tensor([1.0, 0.0], dtype=torch.float32, device=f.device))
            for f in filters]


def covered_filter_update(filters, samples, weights, yf, reg_filters, sample_energy, new_xf, num_iter) -> bool:
    lists = [filters, samples, weights, yf, reg_filters, sample_energy]
    if not 1 <= len(filters) <= _lib.PT_ECO_MAX_BLOCKS or any(len(v) != len(filters) for v in lists) or not 0 <= int(num_iter) <= 62:
        return False
    if new_xf is not None and len(new_xf) != len(filters):
        return False
    for b, f in enumerate(filters):
        if not (covered_series(f) and f.is_contiguous() and f.shape[0] == 1):
            return False
        _, c, Hf, Wh, _ = f.shape
        s, w, y, r, e = samples[b], weights[b], yf[b], reg_filters[b], sample_energy[b]
        if not (_dev_f32(s, 5) and tuple(s.shape[:2]) == (Hf, Wh) and s.shape[3] == c and s.shape[2] <= _lib.PT_ECO_MAX_SAMPLES and c <= 64):
            return False
        if not (_dev_f32(w, 1) and w.numel() == s.shape[2] and _dev_f32(y) and y.numel() == Hf * Wh and _dev_f32(e) and e.numel() == c * Hf * Wh):
            return False
        if not (_dev_f32(r, 4) and r.shape[:2] == (1, 1) and max(r.shape[2:]) <= 15):
            return False
        Rh, Rw = r.shape[2:]
        if min(Rh - 1, Hf - 1) != Rh - 1 or min(Rw - 1, 2 * Wh - 2) != Rw - 1:        # a clipped padding: the reference's conv2d raises there
            return False
        if new_xf is not None and not (covered_series(new_xf[b]) and new_xf[b].shape == f.shape):
            return False
        if not _no_grad_needed(f, s, w, y, r, e):
            return False
    return True


@device_guarded
def filter_update(filters, samples, weights, yf, reg_filters, sample_energy, new_xf, state, num_iter, learning_rates, reg_energy,
                  fletcher_reeves=False, standard_alpha=True, direction_forget_factor=0.0, precond_data_param=0.3, precond_reg_param=0.15):
    """FilterOptim.run for all blocks in one call: `filters` (1, c, Hf, Wh, 2) and `sample_energy` (1, c, Hf, Wh) are updated IN PLACE, `state`
    (new_cg_state) carries p, r_prev and rho between calls.  Definition in include/pt_hot.h."""
    _require_device(*filters)
    if not covered_filter_update(filters, samples, weights, yf, reg_filters, sample_energy, new_xf, num_iter):
        raise NotImplementedError("filter update: contiguous device fp32 blocks, c <= 64, n <= 1024, reg filter <= 15 x 15 with unclipped padding")
    nb = len(filters)
    keep, arr = [], (_lib.EcoFuBlock * nb)()
    for b, f in enumerate(filters):
        _, c, Hf, Wh, _ = f.shape
        ts = [samples[b].contiguous(), weights[b].contiguous(), yf[b].contiguous(), reg_filters[b].contiguous()]
        e = sample_energy[b]
        if not e.is_contiguous():
            raise NotImplementedError("filter update: sample_energy must be contiguous (it is updated in place)")
        nx = new_xf[b].contiguous() if new_xf is not None else None
        keep += ts + [nx]
        arr[b] = _lib.EcoFuBlock(ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), e.data_ptr(),
                                 nx.data_ptr() if nx is not None else None, f.data_ptr(), state[b]["p"].data_ptr(), state[b]["r_prev"].data_ptr(),
                                 state[b]["state"].data_ptr(), Hf, Wh, c, ts[0].shape[2], ts[3].shape[2], ts[3].shape[3],
                                 float(learning_rates[b]), float(reg_energy[b]))
    L = _lib.lib()
    ws = workspace(L.pt_eco_filter_update_ws_bytes(arr, nb), filters[0].device)
    rc = L.pt_eco_filter_update_f32(arr, nb, int(num_iter), int(bool(fletcher_reeves)), int(bool(standard_alpha)), float(direction_forget_factor),
                                    float(precond_data_param), float(precond_reg_param), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_eco_filter_update_f32")
    return filters


def _cg_state_of(opt):
    """The device CG state kept on a reference FilterOptim object (created on first use; the object's own p / rho / r_prev mirror it)."""
    st = getattr(opt, "_amd_cg_state", None)
    if st is None or len(st) != len(opt.filter) or any(s["p"].shape != f.shape or s["p"].device != f.device for s, f in zip(st, opt.filter)):
        st = new_cg_state(opt.filter)
        opt._amd_cg_state = st
    return st


def covered_filter_run(opt, num_iter, new_xf=None) -> bool:
    if opt.debug or opt.sample_energy is None or getattr(opt, "filter", None) is None:
        return False
    if getattr(opt, "p", None) is not None and getattr(opt, "_amd_cg_state", None) is None and opt.direction_forget_factor != 0:
        return False                                  # a direction carried over from the reference's own run: it finishes what it began
    energy = [e for e in opt.sample_energy]
    if not all(isinstance(e, torch.Tensor) for e in energy):
        return False
    return covered_filter_update(list(opt.filter), list(opt.training_samples), list(opt.sample_weights), list(opt.yf), list(opt.reg_filter),
                                 energy, None if new_xf is None else list(new_xf), num_iter)


def tracker_filter_run(opt, num_iter, new_xf=None):
    """FilterOptim.run (optim.py:142-165) of a reference FilterOptim object: `opt.filter` and `opt.sample_energy` are updated in place."""
    if num_iter == 0:
        return
    st = _cg_state_of(opt)
    prm = opt.params
    lrs = [float(v) for v in prm.precond_learning_rate]
    # the reference REBINDS sample_energy (the first one is a permuted view shared with the joint problem): a fresh contiguous tensor per call
    opt.sample_energy = type(opt.filter)([e.clone(memory_format=torch.contiguous_format) for e in opt.sample_energy])
    filter_update(list(opt.filter), list(opt.training_samples), list(opt.sample_weights), list(opt.yf), list(opt.reg_filter),
                  list(opt.sample_energy), None if new_xf is None else list(new_xf), st, num_iter, lrs, [float(v) for v in opt.reg_energy],
                  opt.fletcher_reeves, opt.standard_alpha, opt.direction_forget_factor, prm.precond_data_param, prm.precond_reg_param)
    TL = type(opt.filter)
    opt.p, opt.r_prev, opt.rho = TL([s["p"] for s in st]), TL([s["r_prev"] for s in st]), TL([s["state"][0] for s in st])


# ---------------------------------------------------------------------------------------------------------------------------
# first-frame joint optimisation of filter and projection matrix (GaussNewtonCG.run on FactorizedConvProblem)

def _init_pads(Hf, Wh, Rh, Rw):
    return min(Rh - 1, Hf - 1), min(Rw - 1, Wh - 1)


def _init_reg_fwd(v, reg, left):
    """The ONE correlation of optim.py:52-69: v complex (c, Hf, Wh) extended to the left by its conjugate flip (`left`) or by zeros (the
    Jacobian: the reference detaches the extension) -> real (2 c, 1, H1, W1), the real and imaginary parts as a batch."""
    c, Hf, Wh = v.shape
    p1, p2 = _init_pads(Hf, Wh, *reg.shape[-2:])
    ext = v[:, :, 1:p2 + 1].flip((1, 2)).conj().resolve_conj()
    x = torch.cat((ext if left else torch.zeros_like(ext), v), -1)
    x = torch.view_as_real(x).permute(0, 3, 1, 2).reshape(2 * c, 1, Hf, Wh + p2)
    return torch.nn.functional.conv2d(x, reg.reshape(1, 1, *reg.shape[-2:]), padding=(p1, p2))


def _init_reg_T(g, reg, c, Hf, Wh):
    """Its transpose on the non-detached columns -> complex (c, Hf, Wh)."""
    p1, p2 = _init_pads(Hf, Wh, *reg.shape[-2:])
    x = torch.nn.functional.conv_transpose2d(g, reg.reshape(1, 1, *reg.shape[-2:]), padding=(p1, p2))[..., p2:]
    return torch.view_as_complex(x.reshape(c, 2, Hf, Wh).permute(0, 2, 3, 1).contiguous())


def joint_init_torch(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter, projection_reg):
    """GaussNewtonCG.run(num_cg_iter, num_gn_iter) on FactorizedConvProblem with the Gauss-Newton operator written out (what the two autograd
    passes of the reference compute; definition in include/pt_hot.h), any device, any floating dtype.  `filters` (1, c, Hf, Wh, 2) and
    `projections` (Cin, c) are updated IN PLACE."""
    nb = len(filters)
    if num_cg_iter == 0 or num_gn_iter == 0:
        return filters, projections
    cplx = lambda t: torch.view_as_complex(t.contiguous())      # noqa: E731
    X = [cplx(s) for s in samples]                                # (Hf, Wh, n, Cin)
    sw = [w.reshape(-1) for w in weights_sqrt]
    y = [t.reshape(f.shape[2:4]) for t, f in zip(yf, filters)]
    dM = [d.reshape(f.shape[1:4]) for d, f in zip(diag_M, filters)]
    root = math.sqrt(projection_reg)

    def fwd(b, h, P, dh, dP, left):
        """J (dh, dP) at (h, P); with dP None the residual's own products: (data, reg, proj)"""
        m = dh.permute(1, 2, 0) @ P.t().to(h.dtype)
        if dP is not None:
            m = m + h.permute(1, 2, 0) @ dP.t().to(h.dtype)
        return (X[b] @ m.unsqueeze(-1)).squeeze(-1) * sw[b], _init_reg_fwd(dh, reg_filters[b], left), root * (P if dP is None else dP)

    def transposed(b, h, P, g_data, g_reg, g_proj):
        v = ((g_data * sw[b]).unsqueeze(-2) @ X[b].conj()).squeeze(-2)                   # (Hf, Wh, Cin)
        gh = (v @ P.to(h.dtype)).permute(2, 0, 1) + _init_reg_T(g_reg, reg_filters[b], *h.shape)
        return gh, torch.einsum("hwi,chw->ic", v, h.conj()).real + root * g_proj

    def ip(a, b):
        d = a[0].real * b[0].real + a[0].imag * b[0].imag
        return 2 * d.sum() - d[..., 0].sum() + (a[1] * b[1]).sum()

    for _ in range(num_gn_iter):
        hs, Ps = [cplx(f[0]).clone() for f in filters], [p.clone() for p in projections]
        r = []
        for b in range(nb):
            data, reg, proj = fwd(b, hs[b], Ps[b], hs[b], None, True)
            gh, gP = transposed(b, hs[b], Ps[b], data - sw[b] * y[b].unsqueeze(-1), reg, proj)
            r.append((-gh, -gP))
        p, rho, dx = None, None, None
        for ii in range(num_cg_iter):
            z = [(rh / d, rP / pc) for (rh, rP), d, pc in zip(r, dM, proj_precond)]
            rho1, rho = rho, [ip(rr, zz) for rr, zz in zip(r, z)]
            if any(bool(v == 0) for v in rho):
                break
            if p is None:
                p = z
            else:
                beta = [(n / o).clamp(0) for n, o in zip(rho, rho1)]
                p = [(zh + ph * bt, zP + pP * bt) for (zh, zP), (ph, pP), bt in zip(z, p, beta)]
            q = [transposed(b, hs[b], Ps[b], *fwd(b, hs[b], Ps[b], p[b][0], p[b][1], False)) for b in range(nb)]
            alpha = [rh / ip(pp, qq) for rh, pp, qq in zip(rho, p, q)]
            step = [(ph * al, pP * al) for (ph, pP), al in zip(p, alpha)]
            dx = step if dx is None else [(dh + sh, dP + sP) for (dh, dP), (sh, sP) in zip(dx, step)]
            if ii < num_cg_iter - 1:
                r = [(rh - qh * al, rP - qP * al) for (rh, rP), (qh, qP), al in zip(r, q, alpha)]
        if dx is not None:
            for f, P, (dh, dP) in zip(filters, projections, dx):
                f += torch.view_as_real(dh).unsqueeze(0)
                P += dP
    return filters, projections


INIT_MAX_CIN, INIT_MAX_SAMPLES, INIT_MAX_CG, INIT_MAX_GN = 512, 64, 62, 32


def covered_joint_init(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter) -> bool:
    lists = [filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond]
    if not 1 <= len(filters) <= _lib.PT_ECO_MAX_BLOCKS or any(len(v) != len(filters) for v in lists):
        return False
    if not (isinstance(num_cg_iter, int) and isinstance(num_gn_iter, int) and 0 <= num_cg_iter <= INIT_MAX_CG and 0 <= num_gn_iter <= INIT_MAX_GN):
        return False
    for f, P, s, w, y, r, d in zip(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M):
        if not (covered_series(f) and f.shape[0] == 1 and _dev_f32(P, 2)):
            return False
        _, c, Hf, Wh, _ = f.shape
        if not (_dev_f32(s, 5) and tuple(s.shape[:2]) == (Hf, Wh) and s.shape[-1] == 2 and s.shape[3] == P.shape[0] and P.shape[1] == c):
            return False
        n, Cin = s.shape[2], s.shape[3]
        if not (c <= 64 and 1 <= Cin <= INIT_MAX_CIN and 1 <= n <= INIT_MAX_SAMPLES and Hf * Wh <= 1 << 20):
            return False
        if not (_dev_f32(w) and w.numel() in (1, n) and _dev_f32(y) and y.numel() == Hf * Wh and _dev_f32(d) and d.numel() == c * Hf * Wh):
            return False
        if not (_dev_f32(r) and r.dim() in (2, 4) and r.numel() == r.shape[-2] * r.shape[-1] and max(r.shape[-2:]) <= 15):
            return False
        if not (_no_grad_needed(f, P, s, w, y, r, d) and len({t.device for t in (f, P, s, w, y, r, d)}) == 1):
            return False
    return True


@device_guarded
def joint_init(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter, projection_reg):
    """GaussNewtonCG.run(num_cg_iter, num_gn_iter) on FactorizedConvProblem for all blocks in one call: `filters` (1, c, Hf, Wh, 2) and
    `projections` (Cin, c) are updated IN PLACE (a strided one -- the tracker's projection matrix is a clone of a column slice and keeps
    its strides -- through a dense copy that is written back).  samples (Hf, Wh, n, Cin, 2) uncompressed, weights_sqrt 1 or n entries, yf (Hf, Wh)-shaped,
    reg_filters (Rh, Rw)-shaped, diag_M (c, Hf, Wh)-shaped and proj_precond (a float per block): the problem constructor's preconditioner.
    Definition in include/pt_hot.h."""
    _require_device(*filters)
    if not covered_joint_init(filters, projections, samples, weights_sqrt, yf, reg_filters, diag_M, proj_precond, num_cg_iter, num_gn_iter):
        raise NotImplementedError(f"joint init: device fp32 filters (1, c, Hf, Wh, 2) and projections (Cin, c), c <= 64, Cin <= "
                                  f"{INIT_MAX_CIN}, n <= {INIT_MAX_SAMPLES}, reg filter <= 15 x 15, <= {INIT_MAX_CG} CG x {INIT_MAX_GN} GN iterations")
    nb = len(filters)
    keep, arr = [], (_lib.EcoInitBlock * nb)()
    dense = [(t, t if t.is_contiguous() else t.contiguous()) for t in list(filters) + list(projections)]
    for b, ((_, f), (_, P)) in enumerate(zip(dense[:nb], dense[nb:])):
        _, c, Hf, Wh, _ = f.shape
        ts = [samples[b].contiguous(), weights_sqrt[b].contiguous(), yf[b].contiguous(), reg_filters[b].contiguous(), diag_M[b].contiguous()]
        keep += ts
        arr[b] = _lib.EcoInitBlock(*[t.data_ptr() for t in ts], f.data_ptr(), P.data_ptr(), Hf, Wh, P.shape[0], c, ts[0].shape[2], ts[1].numel(),
                                   ts[3].shape[-2], ts[3].shape[-1], float(proj_precond[b]))
    L = _lib.lib()
    ws = workspace(L.pt_eco_joint_init_ws_bytes(arr, nb), filters[0].device)
    rc = L.pt_eco_joint_init_f32(arr, nb, int(num_gn_iter), int(num_cg_iter), float(projection_reg), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_eco_joint_init_f32")
    for t, d in dense:
        if d is not t:
            t.copy_(d)
    return filters, projections


def _joint_run_args(opt):
    """joint_init's arguments from a reference GaussNewtonCG object on a FactorizedConvProblem (optim.py:9-31); None when the object is
    not of that kind."""
    prob, x = opt.problem, list(opt.x)
    nb = len(x) // 2
    if len(x) != 2 * nb or nb == 0 or getattr(prob, "sample_weights_sqrt", None) is None or len(prob.diag_M) != 2 * nb:
        return None
    if not all(isinstance(t, torch.Tensor) and t.dim() == 5 and t.shape[2:4] == (1, 1) for t in prob.yf):
        return None
    return dict(filters=x[:nb], projections=x[nb:], samples=list(prob.training_samples), weights_sqrt=list(prob.sample_weights_sqrt),
                yf=[t[..., 0] for t in prob.yf], reg_filters=list(prob.reg_filter), diag_M=list(prob.diag_M[:nb]),
                proj_precond=list(prob.diag_M[nb:]))


def covered_joint_run(opt, num_cg_iter, num_gn_iter=None) -> bool:
    """A `run(num_cg_iter, num_gn_iter)` of a GaussNewtonCG built by `gauss_newton_cg` that the kernels take: integer iteration counts of
    at least 1 (zero iterations and lists keep the reference's own behaviour) on an object whose constructor found the kernel route."""
    if not (getattr(opt, "_amd_route", False) and isinstance(num_cg_iter, int) and isinstance(num_gn_iter, int)):
        return False
    if num_cg_iter < 1 or num_gn_iter < 1:
        return False
    a = _joint_run_args(opt)
    return a is not None and covered_joint_init(**a, num_cg_iter=num_cg_iter, num_gn_iter=num_gn_iter)


def tracker_joint_run(opt, num_cg_iter, num_gn_iter=None):
    """GaussNewtonCG.run (optimization.py:328-374) of a reference object: the tracker's `filter` and `projection_matrix` tensors are updated in
    place, as `self.x += delta_x` does; `losses` and `residuals` stay the empty tensors of the constructor (debug is off)."""
    a = _joint_run_args(opt)
    a["proj_precond"] = [float(v) for v in a["proj_precond"]]
    joint_init(**a, num_cg_iter=num_cg_iter, num_gn_iter=num_gn_iter, projection_reg=float(opt.problem.params.projection_reg))
    return opt.losses, opt.residuals


def gauss_newton_cg(ref_cls, problem_cls, on_run=None):
    """The class for the name `pytracking.tracker.eco.eco.GaussNewtonCG` (eco.py:9): a subclass of the reference's `ref_cls` whose
    constructor notes whether the kernels cover the object -- a `problem_cls` (eco.optim.FactorizedConvProblem) on device fp32 tensors,
    debug / analyze / plotting off, the CG settings the tracker uses -- and whose `run` then goes to `tracker_joint_run`; every other object
    and call (a list-valued num_cg_iter, CPU tensors, zero iterations) runs the reference's `run`.  `on_run(fast)` is told which."""
    class GaussNewtonCG(ref_cls):
        __doc__ = ref_cls.__doc__

        def __init__(self, problem, variable, *args, **kw):
            super().__init__(problem, variable, *args, **kw)
            self._amd_route = bool(isinstance(problem, problem_cls) and not self.debug and self.fletcher_reeves and self.standard_alpha
                                   and self.direction_forget_factor == 0 and self.cg_eps == 0
                                   and all(isinstance(t, torch.Tensor) and _dev_f32(t) for t in variable))

        def run(self, num_cg_iter, num_gn_iter=None):
            fast = covered_joint_run(self, num_cg_iter, num_gn_iter)
            if on_run is not None:
                on_run(fast)
            if fast:
                return tracker_joint_run(self, num_cg_iter, num_gn_iter)
            return super().run(num_cg_iter, num_gn_iter)

    return GaussNewtonCG
