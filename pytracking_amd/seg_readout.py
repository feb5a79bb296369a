"""Segmentation read-out of the LWL / RTS trackers on the device (seg_readout.hip): what `LWL.track` / `RTS.track` and their
`merge_results` run on the CPU between the decoder's raw score map and the next frame's label encoder.

    crop_to_image      convert_scores_crop_to_image (pytracking/tracker/lwl/lwl.py:330-359, rts/rts.py:460-493, rts/sta_helper.py:88-117)
                       with `> 0`, sigmoid and the sums of get_target_state / masks_to_bboxes           pt_seg_readout_f32
    state              the same statistics of a probability image that is already on the device        pt_seg_state_f32
    target_state       the host-side decisions of the two get_target_state bodies (lwl.py:276-300, rts.py:405-430) on a statistics block
    merge              merge_results' soft aggregation, arg-max, per-object statistics (lwl.py:217-269) pt_seg_merge_f32
    sample_mask_patch  sample_patch(is_mask=True) (pytracking/features/preprocessing.py:54-148)         pt_sample_mask_patch_f32

The integer decisions -- the resized size, the window's corner, the crop geometry -- are made here on the host with the reference's own
rules (Python's `int()` truncates towards zero); the kernels see integers.  Every function takes and returns device tensors; a read-out
and a merge each live in ONE device buffer, so `to_host` brings all of it over in a single copy.  `merge_results_lwl` / `merge_results_rts`
/ `convert_*` are the bodies `install(seg_readout=True)` binds in place of the reference's methods; they keep the reference's return types.
"""
import collections
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .filter import _ptr, _require_device, _stream, device_guarded, workspace
from .preprocessing import patch_geometry

STATS = _lib.PT_SEG_STATS_FLOATS
MAX_OBJECTS, MAX_DIM = _lib.PT_SEG_MAX_OBJECTS, _lib.PT_SEG_MAX_DIM
# positions of a statistics block (include/pt_hot.h)
PROB_SUM, E_Y, E_X, VAR_Y, VAR_X, CLAMPED, MASK_COUNT, X_MIN, Y_MIN, X_MAX, Y_MAX = 0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14
OUTPUTS = ("scores", "prob", "mask")
FILL = -100.0

Placement = collections.namedtuple("Placement", "Hr Wr r1 c1 r1_pad c1_pad r2_pad c2_pad")


def _align(n, to=64):
    return (int(n) + to - 1) // to * to


def placement(crop_hw, image_hw, sample_scale, sample_pos):
    """The integers of convert_scores_crop_to_image (lwl.py:335-352): F.interpolate's output size for `scale_factor`, the window's
    unclipped corner and the four pads.  `int()` truncates towards zero, as the reference's."""
    s = float(sample_scale)
    Hr, Wr = int(math.floor(float(crop_hw[0]) * s)), int(math.floor(float(crop_hw[1]) * s))
    r1, c1 = int(float(sample_pos[0]) - 0.5 * Hr), int(float(sample_pos[1]) - 0.5 * Wr)
    r2, c2 = r1 + Hr, c1 + Wr
    return Placement(Hr, Wr, r1, c1, max(0, -r1), max(0, -c1), max(r2 - int(image_hw[0]), 0), max(c2 - int(image_hw[1]), 0))


def intersects(pl, image_hw):
    """Does the window meet the image?  (The reference's slice assignment raises when it does not.)"""
    return (pl.Hr > 0 and pl.Wr > 0 and pl.r1 < int(image_hw[0]) and pl.c1 < int(image_hw[1]) and pl.r1 + pl.Hr > 0 and pl.c1 + pl.Wr > 0)


def _same_bits(a, b):
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


class Readout:
    """One read-out in one device buffer: `stats` (16 floats, include/pt_hot.h) and the requested images as views of `flat`."""

    def __init__(self, flat, image_hw, names, pl):
        self.flat, self.image_hw, self.names, self.placement = flat, tuple(image_hw), tuple(names), pl
        self.stats = flat[:STATS]
        n = _align(image_hw[0] * image_hw[1])
        for k, name in enumerate(OUTPUTS):
            setattr(self, name + "_im", None)
        for k, name in enumerate(names):
            setattr(self, name + "_im", flat[64 + k * n:64 + k * n + image_hw[0] * image_hw[1]].view(*image_hw))

    def to_host(self):
        """The whole read-out on the host after ONE copy."""
        return Readout(self.flat.cpu(), self.image_hw, self.names, self.placement)

    def equal(self, other):
        """Bit-equal statistics and images (the buffer's alignment gaps are not compared)."""
        return self.names == other.names and all(_same_bits(getattr(self, n), getattr(other, n)) for n in ("stats",) + tuple(
            n + "_im" for n in self.names))


def _scores2d(scores):
    if scores.dim() < 2 or scores.numel() != scores.shape[-2] * scores.shape[-1]:
        raise NotImplementedError("one score map (..., H, W) with singleton leading dimensions")
    return scores.reshape(scores.shape[-2], scores.shape[-1]).contiguous()


@device_guarded
def crop_to_image(scores, image_hw, sample_scale, sample_pos, outputs=OUTPUTS):
    """Crop scores (.., Hc, Wc) -> Readout on the device: scores_im / prob_im / mask_im (those named in `outputs`) and the statistics block
    of prob_im.  A window that misses the image gives the all-background image (the reference raises there)."""
    _require_device(scores)
    s2 = _scores2d(scores)
    names = tuple(n for n in OUTPUTS if n in outputs)
    if set(outputs) - set(OUTPUTS):
        raise ValueError(f"outputs are named from {OUTPUTS}")
    Hi, Wi = int(image_hw[0]), int(image_hw[1])
    pl = placement(s2.shape, (Hi, Wi), sample_scale, sample_pos)
    if pl.Hr < 1 or pl.Wr < 1:
        raise ValueError("the scale factor resizes the crop to nothing")
    L = _lib.lib()
    need = L.pt_seg_readout_ws_bytes(Hi, Wi)
    if need == 0 or max(s2.shape) > MAX_DIM or max(pl.Hr, pl.Wr, abs(pl.r1), abs(pl.c1)) > MAX_DIM:
        raise NotImplementedError("read-out: size outside the covered range")
    flat = torch.empty(64 + len(names) * _align(Hi * Wi), dtype=torch.float32, device=s2.device)
    out = Readout(flat, (Hi, Wi), names, pl)
    ws = workspace(need, s2.device)
    ptrs = [_ptr(t) if t is not None else None for t in (out.scores_im, out.prob_im, out.mask_im)]
    rc = L.pt_seg_readout_f32(_ptr(s2), s2.shape[0], s2.shape[1], float(sample_scale), pl.Hr, pl.Wr, pl.r1, pl.c1, Hi, Wi, *ptrs,
                              _ptr(out.stats), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_seg_readout_f32")
    return out


@device_guarded
def state(prob, mask=None):
    """Statistics block (16 floats on the device) of a probability image (.., H, W); the mask is `mask` > 0, or prob > 0.5 without one."""
    _require_device(prob, mask)
    p = _scores2d(prob)
    m = None if mask is None else _scores2d(mask)
    if m is not None and m.shape != p.shape:
        raise ValueError("mask and probability image differ in size")
    L = _lib.lib()
    need = L.pt_seg_state_ws_bytes(p.shape[0], p.shape[1])
    if need == 0:
        raise NotImplementedError("state: size outside the covered range")
    stats = torch.empty(STATS, dtype=torch.float32, device=p.device)
    ws = workspace(need, p.device)
    rc = L.pt_seg_state_f32(_ptr(p), None if m is None else _ptr(m), p.shape[0], p.shape[1], _ptr(stats), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_seg_state_f32")
    return stats


def target_state(stats, kind="lwl", pos=None, target_sz=None, min_mask_area=-10, sz_factor=4, seg_to_bb_mode="var"):
    """get_target_state on a statistics block (a device block is copied once): (pos [e_y, e_x], size [sqrt(var_y), sqrt(var_x)] *
    sz_factor) as two CPU tensors, or the caller's (pos, target_sz) where the reference returns the previous state -- LWL: prob_sum <
    min_mask_area (lwl.py:280); RTS: moments of max(p, 0), `not (e_h > 0 and e_w > 0)` (rts.py:408-425)."""
    if seg_to_bb_mode != "var":
        raise Exception('Unknown seg_to_bb_mode mode {}'.format(seg_to_bb_mode))
    if kind not in ("lwl", "rts"):
        raise ValueError("kind is 'lwl' or 'rts'")
    st = torch.as_tensor(stats).detach().reshape(-1).cpu()
    if kind == "lwl":
        if float(st[PROB_SUM]) < min_mask_area:
            return pos, target_sz
        o = 0
    else:
        o = CLAMPED
    e_y, e_x, e_h, e_w = st[o + E_Y], st[o + E_X], st[o + VAR_Y], st[o + VAR_X]
    if kind == "rts" and not (e_h > 0 and e_w > 0):
        return pos, target_sz
    return torch.Tensor([e_y, e_x]), torch.Tensor([e_h.sqrt() * sz_factor, e_w.sqrt() * sz_factor])


def mask_bbox(stats, fmt="t"):
    """masks_to_bboxes (ltr/data/bounding_box_utils.py:33-67) of the block's mask as a list of 4 floats: 'v' [x_min, y_min, x_max, y_max],
    't' [x_min, y_min, w, h], 'c' [x_centre, y_centre, w, h]."""
    st = torch.as_tensor(stats).detach().reshape(-1).cpu()
    x0, y0, x1, y1 = (float(st[k]) for k in (X_MIN, Y_MIN, X_MAX, Y_MAX))
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if fmt == "v":
        return [x0, y0, x1, y1]
    if fmt == "t":
        return [x0, y0, w, h]
    if fmt == "c":
        return [x0 + 0.5 * w, y0 + 0.5 * h, w, h]
    raise ValueError("Undefined bounding box layout '%s'" % fmt)


class Merged:
    """One merge in one device buffer (bytes): `stats` (N, 16), `prob` (N + 1, H, W) background first, `labels` (H, W) uint8."""

    def __init__(self, flat, n, hw):
        self.flat, self.n, self.hw = flat, int(n), tuple(hw)
        H, W = self.hw
        a, b = 4 * _align(self.n * STATS), 4 * _align((self.n + 1) * H * W)
        self.stats = flat[:4 * self.n * STATS].view(torch.float32).view(self.n, STATS)
        self.prob = flat[a:a + 4 * (self.n + 1) * H * W].view(torch.float32).view(self.n + 1, H, W)
        self.labels = flat[a + b:a + b + H * W].view(H, W)

    @staticmethod
    def nbytes(n, hw):
        return 4 * _align(n * STATS) + 4 * _align((n + 1) * hw[0] * hw[1]) + _align(hw[0] * hw[1])

    def to_host(self):
        """The whole merge on the host after ONE copy."""
        return Merged(self.flat.cpu(), self.n, self.hw)

    def equal(self, other):
        """Bit-equal statistics, probabilities and labels (the buffer's alignment gaps are not compared)."""
        return all(_same_bits(getattr(self, n), getattr(other, n)) for n in ("stats", "prob", "labels"))


@device_guarded
def merge(scores):
    """Raw scores (N, H, W) of N objects -> Merged: the soft aggregation of merge_results (lwl.py:228-248), the arg-max label map and per
    object the statistics block of its merged probability with its label region as the mask."""
    _require_device(scores)
    if scores.dim() == 4 and scores.shape[1] == 1:
        scores = scores[:, 0]
    if scores.dim() != 3:
        raise NotImplementedError("merge takes (N, H, W) scores")
    s = scores.contiguous()
    N, H, W = (int(v) for v in s.shape)
    L = _lib.lib()
    need = L.pt_seg_merge_ws_bytes(N, H, W)
    if need == 0:
        raise NotImplementedError(f"merge: 1 to {MAX_OBJECTS} objects, sides up to {MAX_DIM}")
    out = Merged(torch.empty(Merged.nbytes(N, (H, W)), dtype=torch.uint8, device=s.device), N, (H, W))
    ws = workspace(need, s.device)
    rc = L.pt_seg_merge_f32(_ptr(s), N, H, W, _ptr(out.prob), _ptr(out.labels), _ptr(out.stats), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "pt_seg_merge_f32")
    return out


@device_guarded
def sample_mask_patch(im, pos, sample_sz, output_sz=None, mode='replicate', max_scale_change=None):
    """sample_patch(..., is_mask=True) for a device image (1, C, H, W): (patch (1, C, oh, ow), patch_coord (1, 4) on the host).  Zero
    padding, nearest resize with ATen's fp32 index rule; the padded crop itself when it already has the output size."""
    _require_device(im)
    if im.dim() != 4 or im.shape[0] != 1:
        raise NotImplementedError("sample_mask_patch takes one image (1, C, H, W)")
    g, c = patch_geometry(im.shape[-2:], pos, sample_sz, output_sz, mode, max_scale_change)
    oh, ow = (g.crop_h, g.crop_w) if output_sz is None else (int(output_sz[0]), int(output_sz[1]))
    im = im.contiguous()
    C, H, W = (int(v) for v in im.shape[1:])
    out = torch.empty((1, C, oh, ow), dtype=torch.float32, device=im.device)
    rc = _lib.lib().pt_sample_mask_patch_f32(_ptr(im), C, H, W, (_lib.PatchGeom * 1)(g), _ptr(out), oh, ow, _stream())
    _lib.check(rc, "pt_sample_mask_patch_f32")
    return out, torch.tensor([c], dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the bodies install(seg_readout=True) binds in place of the reference's methods
# ---------------------------------------------------------------------------------------------------------------------
def convert_covered(scores, im, sample_scale, sample_pos):
    """Device fp32 scores of one map, a covered size, a window that meets the image (the reference raises otherwise: its call)."""
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() >= 2
            and scores.numel() == scores.shape[-2] * scores.shape[-1] and scores.numel() > 0):
        return False
    hw = tuple(int(v) for v in im.shape[-2:])
    pl = placement(scores.shape[-2:], hw, sample_scale, sample_pos)
    return (max(*scores.shape[-2:], *hw, pl.Hr, pl.Wr, abs(pl.r1), abs(pl.c1)) <= MAX_DIM and min(hw) > 0 and intersects(pl, hw))


def convert_scores_crop_to_image(self, segmentation_scores, im, sample_scale, sample_pos):
    """LWL.convert_scores_crop_to_image / STAHelper.convert_scores_crop_to_image: the (H, W) score image as a CPU tensor."""
    out = crop_to_image(segmentation_scores, im.shape[-2:], float(sample_scale), (float(sample_pos[0]), float(sample_pos[1])),
                        outputs=("scores",))
    return out.scores_im.cpu()


def sample_location(self, sample_coords):
    """get_sample_location (rts.py:432-437) in the reference's float32 arithmetic."""
    sc = torch.as_tensor(sample_coords).detach().cpu().float()
    sample_pos = 0.5 * (sc[:2] + sc[2:] - 1)
    sample_scale = ((sc[2:] - sc[:2]) / self.img_sample_sz.cpu()).prod().sqrt()
    return sample_pos, sample_scale


def convert_seg_scores_crop_to_image(self, segmentation_scores, im, sample_coords):
    """RTS.convert_seg_scores_crop_to_image: (score image on the CPU, first row, first column of the window inside the image, rows and
    columns of the resized crop)."""
    sample_pos, sample_scale = sample_location(self, sample_coords)
    out = crop_to_image(segmentation_scores, im.shape[-2:], sample_scale.item(), (sample_pos[0].item(), sample_pos[1].item()),
                        outputs=("scores",))
    pl = out.placement
    return out.scores_im.cpu(), pl.r1 + pl.r1_pad, pl.c1 + pl.c1_pad, pl.Hr, pl.Wr


def _stacked_scores(out_all):
    """merge_results' own stacking (lwl.py:218-228): raw scores, or (mask - 0.5) * 200 for an object on its first frame."""
    maps = []
    for out in out_all.values():
        if 'segmentation_raw' in out.keys():
            maps.append(out['segmentation_raw'])
        else:
            maps.append((out['segmentation'] - 0.5) * 200.0)
    return np.stack(maps)


def merge_covered(self, out_all):
    """1 to 16 objects with distinct ids 1 .. 255, 2-D maps of one covered size, and a tracker that runs on the GPU."""
    try:
        ids = [int(k) for k in out_all.keys()]
        dev = torch.device(getattr(self.params, "device", "cuda" if getattr(self.params, "use_gpu", True) else "cpu"))
        if not (torch.cuda.is_available() and dev.type == "cuda" and 1 <= len(ids) <= MAX_OBJECTS and len(set(ids)) == len(ids)
                and all(0 < k < 256 for k in ids)):
            return False
        shapes = {np.shape(o['segmentation_raw'] if 'segmentation_raw' in o else o['segmentation']) for o in out_all.values()}
        return len(shapes) == 1 and all(len(s) == 2 and 0 < min(s) and max(s) <= MAX_DIM for s in shapes)
    except Exception:
        return False


def _merge_results(self, out_all, kind):
    obj_ids = list(out_all.keys())
    dev = torch.device(getattr(self.params, "device", "cuda"))
    scores = torch.from_numpy(_stacked_scores(out_all)).float().to(dev)                    # one upload
    m = merge(scores).to_host()                                                            # one download
    prob, labels = m.prob.numpy(), m.labels.numpy()
    obj_ids_all = np.array([0, *map(int, obj_ids)], dtype=np.uint8)
    out_merged = OrderedDict()
    out_merged['segmentation'] = obj_ids_all[labels]
    out_merged['segmentation_raw'] = OrderedDict({key: prob[i + 1] for i, key in enumerate(obj_ids)})
    out_first = list(out_all.values())[0]
    for key in out_first.keys():
        if 'segmentation' in key or (kind == "rts" and 'clf_search_area' in key):
            pass
        elif 'target_bbox' in key:
            merged_boxes = {}
            for i, obj_id in enumerate(obj_ids):
                if kind == "lwl":
                    pred_pos, pred_target_sz = target_state(m.stats[i], "lwl", self.pos, self.target_sz, self.params.get('min_mask_area', -10),
                                                            self.params.get('seg_to_bb_sz_factor', 4), self.params.get('seg_to_bb_mode'))
                    new_state = torch.cat((pred_pos[[1, 0]] - (pred_target_sz[[1, 0]] - 1) / 2, pred_target_sz[[1, 0]]))
                    merged_boxes[obj_id] = new_state.tolist()
                else:
                    merged_boxes[obj_id] = mask_bbox(m.stats[i], "t")
            out_merged['target_bbox'] = merged_boxes
        else:
            out_merged[key] = {obj_id: out[key] for obj_id, out in out_all.items()}
    return out_merged


def merge_results_lwl(self, out_all):
    """LWL.merge_results (lwl.py:210-274): the same dictionary, keys and dtypes; boxes from the merged probabilities' moments."""
    return _merge_results(self, out_all, "lwl")


def merge_results_rts(self, out_all):
    """RTS.merge_results (rts.py:340-403): the same dictionary, keys and dtypes; boxes from the label regions."""
    return _merge_results(self, out_all, "rts")
