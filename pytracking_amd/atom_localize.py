"""Host-side mirror of ATOM's per-frame score localisation (include/pt_loc.h, csrc_loc/atom_localize.hip): what `ATOM.localize_target`
and `ATOM.localize_advanced` (pytracking/tracker/atom/atom.py:304-406) do between classification and box refinement -- the Fourier
interpolation of the raw scores onto the output grid, the output window, both peaks and the outcome -- in two launches and ONE host wait.

Two ways in:

`localize(scores, state, window=None)` for callers that own their frame loop: `state` is a `pt_loc_atom_state` block (`state_block(...)`
from explicit values, `tracker_state(tracker, S)` from an ATOM object).  Returns a `Result`.

`covered_localize_target` / `tracker_localize_target`: the (covered, fast) pair `install(atom_localize=True)` binds in place of
`pytracking.tracker.atom.atom.ATOM.localize_target`.  The fast method returns the reference's 4-tuple: `translation_vec` (CPU float32
tensor of 2), `scale_ind` (0-dim CPU int64 tensor: `sample_scales[scale_ind]` at atom.py:252 indexes a host tensor, which torch 2 refuses
for a device index), the (S, 1, G_h, G_w) device score map and the flag (None / 'hard_negative' / 'uncertain' / 'not_found').

Calls the kernels do not cover -- CPU or non-float32 scores, more than one feature block, `debug >= 2`, sizes outside include/pt_loc.h -- go
to the reference method (or raise under `install(strict=True)`).  That fallback still needs `torch.rfft` / `torch.irfft`, which the
installed torch does not have: it works only together with `install(eco=True)`, whose Fourier tools stand in for them.

Still the reference's Python in `ATOM.track` with this installed: `torch.max(score_map).item()` (atom.py:257), `update_state` and the
memory update.
"""
import collections
import ctypes

import torch

from . import _lib_loc as _L
from .filter import _ptr, _stream, device_guarded

# what the reference method returns for each outcome code (PT_AL_NORMAL ... PT_AL_NOT_FOUND)
RETURN_FLAG = (None,) + tuple(_L.FLAGS[1:])

# translation_vec / scale_ind / scores / flag: the reference's 4-tuple; the rest is the record (cells as [row, col] lists)
Result = collections.namedtuple("Result", "translation_vec scale_ind scores flag code peak1 max1 peak2 max2 pick")


def state_block(*, kernel_size, output_sz, img_support_sz, target_sz, target_scale, target_not_found_threshold=0.0, distractor_threshold=0.0,
                hard_negative_threshold=0.0, target_neighborhood_scale=0.0, dispalcement_scale=0.0, translation_weight=1.0,
                scale_factors=(1.0,), advanced_localization=False, windowed=False, hn_without_windowing=False):
    """`pt_loc_atom_state` from explicit values, unprocessed: the float32 arithmetic on them happens inside the library in the reference's
    operation order."""
    st = _L.LocAtomState()
    st.target_not_found_threshold = float(target_not_found_threshold)
    st.distractor_threshold = float(distractor_threshold)
    st.hard_negative_threshold = float(hard_negative_threshold)
    st.target_neighborhood_scale = float(target_neighborhood_scale)
    st.dispalcement_scale = float(dispalcement_scale)
    st.translation_weight = float(translation_weight)
    st.target_scale = float(target_scale)
    st.img_support_sz[:] = [float(v) for v in img_support_sz]
    st.output_sz[:] = [float(v) for v in output_sz]
    st.target_sz[:] = [float(v) for v in target_sz]
    sf = [float(v) for v in scale_factors][:_L.PT_AL_MAX_SCALES]
    st.scale_factors[:] = sf + [1.0] * (_L.PT_AL_MAX_SCALES - len(sf))
    st.kernel_size[:] = [int(v) for v in kernel_size]
    st.advanced_localization = int(bool(advanced_localization))
    st.windowed = int(bool(windowed))
    st.hn_without_windowing = int(bool(hn_without_windowing))
    return st


def _floats(v):
    return v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else [float(x) for x in v]


def tracker_state(tracker):
    """`pt_loc_atom_state` read from an ATOM object exactly as the reference method reads it."""
    prm = tracker.params
    adv = bool(prm.get('advanced_localization', False))
    ts = tracker.target_scale
    return state_block(
        kernel_size=[int(k) for k in tracker.kernel_size[0]], output_sz=_floats(tracker.output_sz), img_support_sz=_floats(tracker.img_support_sz),
        target_sz=_floats(tracker.target_sz), target_scale=ts.item() if isinstance(ts, torch.Tensor) else ts,
        target_not_found_threshold=prm.target_not_found_threshold if adv else 0.0, distractor_threshold=prm.distractor_threshold if adv else 0.0,
        hard_negative_threshold=prm.hard_negative_threshold if adv else 0.0, target_neighborhood_scale=prm.target_neighborhood_scale if adv else 0.0,
        dispalcement_scale=prm.dispalcement_scale if adv else 0.0, translation_weight=tracker.fparams.attribute('translation_weight', 1.0)[0],
        scale_factors=_floats(prm.scale_factors), advanced_localization=adv, windowed=tracker.output_window is not None,
        hn_without_windowing=prm.get('perform_hn_without_windowing', False))


def covered_shape(S, Nh, Nw, Gh, Gw):
    """What the library would refuse on the sizes alone (nothing launched)."""
    return _L.lib().pt_loc_atom_ws_bytes(int(S), int(Nh), int(Nw), int(Gh), int(Gw)) > 0


class _Context:
    """Per device: the pinned result record, its sequence number and the workspace."""

    def __init__(self, device):
        t = torch.zeros(_L.PT_AL_REC_FLOATS, dtype=torch.float32).pin_memory()
        self.rec, self.host, self.rec_ptr = t, t.numpy(), ctypes.c_void_p(t.data_ptr())
        self.seq = 0.0
        self.ws = torch.empty(_L.PT_AL_MAX_SCALES * ((_L.PT_AL_MAX_GRID + _L.PT_AL_BAND_ROWS - 1) // _L.PT_AL_BAND_ROWS) * 16 + 256,
                              dtype=torch.uint8, device=device)


_CONTEXTS = {}


def _context(device):
    if device not in _CONTEXTS:
        _CONTEXTS[device] = _Context(device)
    return _CONTEXTS[device]


class Pending:
    """A queued localisation; wait() is the call's one host wait."""

    def __init__(self, ctx, seq, maps, maps_hn):
        self.ctx, self.seq, self.maps, self.maps_hn, self.result = ctx, seq, maps, maps_hn, None

    def wait(self):
        if self.result is None:
            ctx = self.ctx
            if self.seq != ctx.seq:
                raise RuntimeError("atom_localize: a later call has been queued on this device's record buffer")
            _L.check(_L.lib().pt_loc_atom_wait_f32(ctx.rec_ptr, self.seq, ctypes.c_void_p(torch.cuda.current_stream(self.maps.device).cuda_stream)),
                     "pt_loc_atom_wait_f32")
            v = ctx.host.tolist()
            code = int(v[_L.PT_AL_R_FLAG])
            cell = lambda k: [int(v[k]), int(v[k + 1])]
            self.result = Result(
                translation_vec=torch.tensor(v[_L.PT_AL_R_TV:_L.PT_AL_R_TV + 2], dtype=torch.float32),
                scale_ind=torch.tensor(int(v[_L.PT_AL_R_SCALE]), dtype=torch.int64),
                scores=self.maps_hn if v[_L.PT_AL_R_WHICH] else self.maps, flag=RETURN_FLAG[code], code=code,
                peak1=cell(_L.PT_AL_R_ROW1), max1=v[_L.PT_AL_R_MAX1], peak2=cell(_L.PT_AL_R_ROW2), max2=v[_L.PT_AL_R_MAX2], pick=int(v[_L.PT_AL_R_PICK]))
        return self.result


@device_guarded
def queue(scores, state, window=None):
    """Queue both launches on the current stream; returns a Pending, or None when the library refuses the sizes (nothing queued then).
    scores (S, 1, N_h, N_w) device float32; window (..., G_h, G_w) device float32 when state.windowed."""
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32):
        raise RuntimeError("pytracking_amd ops run on the MI355X only, in fp32")
    if scores.dim() != 4 or scores.shape[1] != 1:
        return None
    S, _, Nh, Nw = scores.shape
    Gh, Gw = int(state.output_sz[0]), int(state.output_sz[1])
    if (Gh, Gw) != (state.output_sz[0], state.output_sz[1]) or not covered_shape(S, Nh, Nw, Gh, Gw):
        return None
    if state.windowed and (window is None or not window.is_cuda or window.dtype != torch.float32 or window.numel() != Gh * Gw
                           or tuple(window.shape[-2:]) != (Gh, Gw)):
        return None
    prm = _L.LocAtomParams()
    _L.check(_L.lib().pt_loc_atom_constants_f32(ctypes.byref(state), ctypes.byref(prm)), "pt_loc_atom_constants_f32")
    ctx = _context(scores.device)
    src = scores if scores.is_contiguous() else scores.contiguous()
    win = None if not state.windowed else (window if window.is_contiguous() else window.contiguous())
    maps = torch.empty(S, 1, Gh, Gw, dtype=torch.float32, device=scores.device)
    maps_hn = torch.empty_like(maps) if (prm.advanced and prm.hn) else None
    ctx.seq = ctx.seq + 1.0 if ctx.seq < 8388607.0 else 1.0
    rc = _L.lib().pt_loc_atom_f32(_ptr(src), S, Nh, Nw, Gh, Gw, None if win is None else _ptr(win), ctypes.byref(prm), _ptr(maps),
                                  None if maps_hn is None else _ptr(maps_hn), ctx.rec_ptr, ctx.seq, _ptr(ctx.ws), ctx.ws.numel(), _stream())
    if rc == _L.PT_AL_ERR_UNSUPPORTED:
        return None
    _L.check(rc, "pt_loc_atom_f32")
    return Pending(ctx, ctx.seq, maps, maps_hn)


def localize(scores, state, window=None):
    """The whole localisation of one frame: a `Result` after one wait."""
    pending = queue(scores, state, window)
    if pending is None:
        raise NotImplementedError("atom_localize: sizes outside the gfx950 localisation (include/pt_loc.h)")
    return pending.wait()


# ---------------------------------------------------------------------------------------------------------------------------------
# drop-in for the unmodified ATOM class: the (covered, fast) pair of install._dispatcher
# ---------------------------------------------------------------------------------------------------------------------------------
def _single(scores_raw):
    if isinstance(scores_raw, torch.Tensor):
        return scores_raw
    return scores_raw[0] if isinstance(scores_raw, (list, tuple)) and len(scores_raw) == 1 else None


def covered_localize_target(self, scores_raw):
    s = _single(scores_raw)
    if s is None or not (isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.float32 and s.dim() == 4 and s.shape[1] == 1):
        return False
    if self.params.debug >= 2 or len(self.kernel_size) != 1 or len(self.feature_sz) != 1:
        return False
    if [int(v) for v in self.feature_sz[0]] != list(s.shape[-2:]) or len(self.params.scale_factors) < s.shape[0]:
        return False
    out = _floats(self.output_sz)
    w = self.output_window
    if len(out) != 2 or any(v != int(v) for v in out) or not covered_shape(s.shape[0], s.shape[2], s.shape[3], out[0], out[1]):
        return False
    return w is None or (w.is_cuda and w.dtype == torch.float32 and tuple(w.shape[-2:]) == (int(out[0]), int(out[1])) and w.numel() == int(out[0] * out[1]))


def tracker_localize_target(self, scores_raw):
    """(translation_vec, scale_ind, scores, flag) of atom.py:304-406, one wait."""
    r = localize(_single(scores_raw), tracker_state(self), self.output_window)
    return r.translation_vec, r.scale_ind, r.scores, r.flag
