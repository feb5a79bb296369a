"""Host-side mirror of the TaMOs per-frame multi-object read-out (include/pt_mot.h, csrc_mot/mot_readout.hip): what
`TaMOs.track` (pytracking/tracker/tamos/tamos.py:155-239) does per object with the outputs of `classify_target`.

Two ways in:

`MotReadout(tracker).run(scores_raw, bbox_preds, sample_coords, image_hw)` for callers that own their frame loop: the whole decision of
every active object -- the map at the regressor's size (bicubic upsample and sigmoid where the reference applies them), both peaks,
the outcome of `localize_advanced`, the box of `direct_bbox_regression` and its clipped form -- in ONE launch and ONE wait.  It reads the
tracker object exactly as the reference methods do (`params`, `pos`, `pos_prev`, `target_sz`, `object_ids`, `img_support_sz`,
`img_sample_sz`, `train_img_sample_sz`, `kernel_size`, `scale_factor`).

Drop-ins for the unmodified class, bound by `install(tamos_readout=True)`: `classify_target` calls the reference method and queues the
read-out of all active objects on the two tensors it returns; `localize_target` and `direct_bbox_regression` return that object's values
from the stash (the first call of the frame is the frame's one wait); `encode_bbox` and `get_label_function` build the training targets
on the device.  Whatever the stash does not cover goes to the reference method.

Still per object in `track()` itself, untouched: `scores_raw[:, :, oid-1].max() > conf_ths` (tamos.py:198) and
`score_map.max().cpu().item()` (tamos.py:216).
"""
import collections
import ctypes
import math

import torch

from . import _lib_mot as _M
from .filter import _ptr, _stream, device_guarded

_NEG_INF = -float("inf")

# One object's results.  score_loc / bbox_raw / bbox: CPU float32 tensors as the reference returns them ([row, col]; x, y, w, h).
Result = collections.namedtuple("Result", "flag score_loc pick max1 peak1 max2 peak2 presence bbox_raw bbox ltrb second")


def frame_block(tracker, sample_coords, image_hw, stride=8, fr=None):
    """`pt_mot_frame`: the host values one frame's read-out reads from the tracker, unprocessed -- the float32 arithmetic on them happens
    inside the library in the reference's operation order.  Optional thresholds the parameter file does not define are -inf."""
    prm = tracker.params
    fr = _M.MotFrame() if fr is None else fr
    fr.target_not_found_threshold = prm.target_not_found_threshold
    fr.uncertain_threshold = prm.get('uncertain_threshold', _NEG_INF)
    fr.hard_sample_threshold = prm.get('hard_sample_threshold', _NEG_INF)
    fr.distractor_threshold = prm.distractor_threshold
    fr.hard_negative_threshold = prm.hard_negative_threshold
    fr.target_neighborhood_scale = prm.target_neighborhood_scale
    fr.dispalcement_scale = prm.dispalcement_scale
    fr.scale_factor = tracker.scale_factor
    fr.img_support_sz[:] = tracker.img_support_sz.tolist()
    fr.img_sample_sz[:] = tracker.img_sample_sz.tolist()
    fr.train_img_sample_sz[:] = tracker.train_img_sample_sz.tolist()
    fr.kernel_size[:] = tracker.kernel_size.tolist() if isinstance(tracker.kernel_size, torch.Tensor) else list(tracker.kernel_size)
    fr.sample_coords[:] = sample_coords.reshape(-1, 4)[0].tolist() if isinstance(sample_coords, torch.Tensor) else list(sample_coords)
    fr.image_h, fr.image_w = int(image_hw[0]), int(image_hw[1])
    fr.stride = int(stride)
    fr.min_width, fr.min_height = 10, 10                             # the defaults of clip_bbox_to_image_area, which track() uses
    fr.normalize_scores = int(bool(prm.get('normalize_scores', False)))
    fr.score_preprocess = 0 if prm.get('score_preprocess', 'none') == 'none' else 1
    fr.score_filter_ksz = int(prm.get('score_filter_ksz', 1))
    fr.window_output = int(bool(prm.get('window_output', False)))
    fr.advanced_localization = int(bool(prm.get('advanced_localization', False)))
    return fr


def covered_configuration(tracker):
    """What the library would refuse on the configuration alone, decided on the host."""
    prm = tracker.params
    ks = tracker.kernel_size.tolist() if isinstance(tracker.kernel_size, torch.Tensor) else list(tracker.kernel_size)
    return (prm.get('score_preprocess', 'none') == 'none' and prm.get('score_filter_ksz', 1) <= 1 and not prm.get('window_output', False)
            and bool(prm.get('advanced_localization', False)) and all((k + 1) % 2 == 0 for k in ks)
            and 1 <= len(tracker.object_ids) <= _M.PT_MOT_MAX_OBJECTS)


class Pending:
    """A queued read-out: what it was queued on, and after wait() the results by object id."""

    def __init__(self, owner, seq, active, oids, scores, bbox, frame, H, W, frame_num):
        self.owner, self.seq, self.active, self.oids = owner, seq, active, oids
        self.scores, self.bbox, self.frame, self.H, self.W, self.frame_num = scores, bbox, frame, H, W, frame_num
        self.results = None
        self.current = None                                          # the object localize_target answered last

    def wait(self):
        if self.results is None:
            self.results = self.owner._collect(self)
        return self.results


class MotReadout:
    def __init__(self, tracker):
        self.tracker = tracker
        self._rec = None
        self._seq = 0.0

    def _record(self):
        if self._rec is None:
            t = torch.zeros(_M.PT_MOT_MAX_OBJECTS, _M.PT_MOT_REC_FLOATS, dtype=torch.float32).pin_memory()
            self._rec = (t, t.numpy(), ctypes.c_void_p(t.data_ptr()))
        return self._rec

    @device_guarded
    def queue(self, scores_raw, bbox_preds, sample_coords, image_hw, stride=8, map_out=None):
        """Queue the read-out of every active object; returns a Pending, or None when the library refuses (nothing queued then).
        scores_raw (..., T, Hs, Ws) raw classifier output, bbox_preds (..., T, 4, H, W), both on the device; map_out: optional (T, H, W)."""
        trk = self.tracker
        if not (scores_raw.is_cuda and bbox_preds.is_cuda and scores_raw.dtype == bbox_preds.dtype == torch.float32):
            raise RuntimeError("pytracking_amd ops run on the MI355X only, in fp32")
        T, four, H, W = bbox_preds.shape[-4:]
        Hs, Ws = scores_raw.shape[-2:]
        if four != 4 or bbox_preds.numel() != T * 4 * H * W or scores_raw.numel() != T * Hs * Ws:
            return None
        oids = [int(o) for o in trk.object_ids]
        if not oids or len(oids) > _M.PT_MOT_MAX_OBJECTS or any(o < 1 or o > T for o in oids):
            return None
        scores = scores_raw if scores_raw.is_contiguous() else scores_raw.contiguous()
        bbox = bbox_preds if bbox_preds.is_contiguous() else bbox_preds.contiguous()
        fr = frame_block(trk, sample_coords, image_hw, stride)
        n = len(oids)
        active = (ctypes.c_int * n)(*[o - 1 for o in oids])
        objs = (_M.MotObject * n)()
        for ob, o in zip(objs, oids):
            ob.pos[:] = trk.pos[o].tolist()
            ob.pos_prev[:] = trk.pos_prev[o].tolist()
            ob.target_sz[:] = trk.target_sz[o].tolist()
        _, _, rec_ptr = self._record()
        self._seq = self._seq + 1.0 if self._seq < 8388607.0 else 1.0
        rc = _M.lib().pt_mot_readout_f32(_ptr(scores), Hs, Ws, _ptr(bbox), H, W, T, active, n, objs, ctypes.byref(fr),
                                         None if map_out is None else _ptr(map_out), rec_ptr, self._seq, _stream())
        if rc == _M.PT_MOT_ERR_UNSUPPORTED:
            return None
        _M.check(rc, "pt_mot_readout_f32")
        return Pending(self, self._seq, active, oids, scores_raw, bbox_preds, fr, H, W, getattr(trk, "frame_num", None))

    def _collect(self, pending):
        """The one wait of the frame: polls the sequence words of the active objects' records, then reads them."""
        if pending.seq != self._seq:
            raise RuntimeError("MotReadout: a later read-out has been queued on this tracker's record buffer")
        _, host, rec_ptr = self._record()
        _M.check(_M.lib().pt_mot_wait_f32(rec_ptr, pending.active, len(pending.oids), pending.seq,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "pt_mot_wait_f32")
        out = collections.OrderedDict()
        block = host.copy()                                          # private copy of all records: scalars through numpy, tensors as views of it
        rows = torch.from_numpy(block)
        R = _M
        for o in pending.oids:
            v, r = block[o - 1].tolist(), rows[o - 1]
            out[o] = Result(flag=_M.FLAGS[int(v[R.PT_MOT_R_FLAG])], score_loc=r[R.PT_MOT_R_ROW:R.PT_MOT_R_ROW + 2],
                            pick=int(v[R.PT_MOT_R_PICK]), max1=v[R.PT_MOT_R_MAX1], peak1=r[R.PT_MOT_R_ROW1:R.PT_MOT_R_ROW1 + 2],
                            max2=v[R.PT_MOT_R_MAX2], peak2=r[R.PT_MOT_R_ROW2:R.PT_MOT_R_ROW2 + 2],
                            presence=v[R.PT_MOT_R_PRESENCE], bbox_raw=r[R.PT_MOT_R_RAW_BOX:R.PT_MOT_R_RAW_BOX + 4],
                            bbox=r[R.PT_MOT_R_BOX:R.PT_MOT_R_BOX + 4], ltrb=r[R.PT_MOT_R_LTRB:R.PT_MOT_R_LTRB + 4],
                            second=bool(v[R.PT_MOT_R_SECOND]))
        return out

    def run(self, scores_raw, bbox_preds, sample_coords, image_hw, stride=8, map_out=None):
        """{object id: Result} of every active object after one wait."""
        pending = self.queue(scores_raw, bbox_preds, sample_coords, image_hw, stride, map_out)
        if pending is None:
            raise NotImplementedError("MotReadout: configuration or shapes outside the gfx950 read-out")
        return pending.wait()


# ---------------------------------------------------------------------------------------------------------------------------------
# training targets
# ---------------------------------------------------------------------------------------------------------------------------------
@device_guarded
def encode_boxes(boxes, image_sample_size, stride):
    """encode_bbox (tamos.py:114-153) for any leading shape: boxes (..., 4) xywh on the device -> (..., 4, H3, W3), one launch."""
    if not (boxes.is_cuda and boxes.dtype == torch.float32 and boxes.shape[-1] == 4):
        raise RuntimeError("pytracking_amd ops run on the MI355X only, in fp32")
    out_h, out_w, stride = int(image_sample_size[0]), int(image_sample_size[1]), int(stride)
    b = boxes.reshape(-1, 4)
    b = b if b.is_contiguous() else b.contiguous()
    out = torch.empty(*boxes.shape[:-1], 4, out_h // stride, out_w // stride, dtype=torch.float32, device=boxes.device)
    _M.check(_M.lib().pt_mot_targets_f32(_ptr(b), b.shape[0], out_h, out_w, stride, _ptr(out), None, None, 0, None, _stream()),
             "pt_mot_targets_f32")
    return out


def label_block(feature_sz, sigma, end_pad):
    lab = _M.MotLabel()
    lab.sz[:] = [float(v) for v in feature_sz]
    lab.sigma[:] = [float(v) for v in sigma]
    lab.end_pad[:] = [float(v) for v in end_pad]
    return lab


def gaussian_labels(centres, feature_sz, sigma, end_pad, device):
    """dcf.label_function_spatial (dcf.py:48-59) for n centres [row, col] (host values) -> (n, LH, LW) on `device`, one launch."""
    lab = label_block(feature_sz, sigma, end_pad)
    flat = [float(v) for c in centres for v in c]
    n = len(flat) // 2
    LH, LW = (int(math.ceil(lab.sz[d] + lab.end_pad[d])) for d in range(2))
    out = torch.empty(n, LH, LW, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _M.check(_M.lib().pt_mot_targets_f32(None, 0, 0, 0, 0, None, ctypes.byref(lab), (ctypes.c_float * (2 * n))(*flat), n, _ptr(out),
                                             _stream()), "pt_mot_targets_f32")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# drop-ins for the unmodified TaMOs class: (covered, fast) pairs for install._dispatcher
# ---------------------------------------------------------------------------------------------------------------------------------
_STASH = "_pt_mot_pending"


def _on_device(tracker):
    return torch.device(tracker.params.device).type == "cuda"


def _readout_of(tracker):
    ro = getattr(tracker, "_pt_mot_readout", None)
    if ro is None:
        ro = tracker._pt_mot_readout = MotReadout(tracker)
    return ro


def make_classify_target(ref):
    def covered(self, sample_x):
        return _on_device(self) and covered_configuration(self)

    def fast(self, sample_x):
        """The reference method, then the read-out of all active objects queued on the two tensors it returns."""
        target_scores, bbox_preds = ref(self, sample_x)
        setattr(self, _STASH, None)
        if target_scores.is_cuda and target_scores.dtype == torch.float32:
            # what extract_backbone_features hands track() as sample_coords (tamos.py:454), and the image size of initialize()
            coords = torch.Tensor([[0, 0, self.img_sample_sz[0] / self.scale_factor, self.img_sample_sz[1] / self.scale_factor]])
            setattr(self, _STASH, _readout_of(self).queue(target_scores, bbox_preds, coords, self.image_sz.tolist(), stride=8))
        return target_scores, bbox_preds
    return covered, fast


def _stashed(self, obj_id, H, W):
    p = getattr(self, _STASH, None)
    if p is None or p.frame_num != self.frame_num or (p.H, p.W) != (H, W) or obj_id not in p.oids:
        return None
    return p


def make_localize_target(ref):
    def covered(self, scores, scale_factor, obj_id):
        p = _stashed(self, obj_id, *scores.shape[-2:])
        return p is not None and scale_factor == self.scale_factor and scores.dim() == 4 and tuple(scores.shape[:2]) == (1, 1)

    def fast(self, scores, scale_factor, obj_id):
        """(scale_ind, scores.squeeze(1), flag, max_disp) of tamos.py:324-429 from the frame's stash; the first call waits."""
        p = getattr(self, _STASH)
        r = p.wait()[obj_id]
        p.current = obj_id
        return torch.zeros((), dtype=torch.int64), scores.squeeze(1), r.flag, r.score_loc.clone()
    return covered, fast


def make_direct_bbox_regression(ref):
    def covered(self, bbox_preds, sample_coords, score_loc, scores_raw, stride=16):
        p = getattr(self, _STASH, None)
        if p is None or p.frame_num != self.frame_num or p.current is None or p.results is None:
            return False
        item = p.bbox.element_size() * 4 * p.H * p.W
        return (stride == p.frame.stride and bbox_preds.is_cuda and bbox_preds.is_contiguous() and bbox_preds.numel() == 4 * p.H * p.W
                and p.bbox.is_contiguous() and bbox_preds.data_ptr() == p.bbox.data_ptr() + (p.current - 1) * item
                and tuple(scores_raw.shape[-2:]) == (p.H, p.W) and sample_coords.reshape(-1, 4)[0].tolist() == list(p.frame.sample_coords)
                and score_loc.int().tolist() == p.results[p.current].score_loc.int().tolist())

    def fast(self, bbox_preds, sample_coords, score_loc, scores_raw, stride=16):
        """torch.Tensor([x1, y1, w, h]) of tamos.py:248-280 for the object localize_target answered last."""
        p = getattr(self, _STASH)
        return p.results[p.current].bbox_raw.clone()
    return covered, fast


def make_encode_bbox(ref):
    def covered(self, bboxes):
        stride, out = self.params.get('feature_stride'), self.params.get('image_sample_size')
        return (isinstance(bboxes, torch.Tensor) and bboxes.is_cuda and bboxes.dtype == torch.float32 and bboxes.dim() == 2
                and bboxes.shape[1] == 4 and bboxes.shape[0] > 0 and isinstance(stride, int) and stride > 0
                and all(isinstance(v, int) and v > 0 and v % stride == 0 for v in out))

    def fast(self, bboxes):
        return encode_boxes(bboxes, self.params.get('image_sample_size'), self.params.get('feature_stride'))
    return covered, fast


def make_get_label_function(ref, TensorList):
    def covered(self, pos, scale_factor):
        return _on_device(self) and isinstance(pos, torch.Tensor) and not pos.is_cuda

    def fast(self, pos, scale_factor):
        """get_label_function (tamos.py:582-592): the centre on the host in the reference's expressions, the Gaussian on the device."""
        target_center_norm = (pos * scale_factor - self.img_support_sz / 2) / self.img_support_sz
        ksz_even = torch.Tensor([(self.kernel_size[0] + 1) % 2, (self.kernel_size[1] + 1) % 2])
        center = self.feature_sz * target_center_norm + 0.5 * ksz_even
        y = gaussian_labels([center.tolist()], self.feature_sz.tolist(), self.sigma.tolist(), ksz_even.tolist(), torch.device(self.params.device))
        return TensorList([y.reshape(1, 1, *y.shape[-2:])])
    return covered, fast
