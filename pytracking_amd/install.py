"""Install the MI355X hot path behind the reference's own Python call boundary.

    import pytracking_amd.install as amd
    amd.install()                     # before the tracker / network is constructed
    # ... `pytracking.tracker.dimp.DiMP`, `atom.ATOM` etc. now run unchanged on top of libpt_hot.so

What gets rebound (import path = contract; nothing in the reference tree is edited):

  ltr.models.layers.filter.apply_filter / apply_feat_transpose / filter_gradient      -> pytracking_amd.filter
  ltr.models.target_classifier.optimizer.{DiMPSteepestDescentGN, DiMPL2SteepestDescentGN,
                                           PrDiMPSteepestDescentNewton}               -> pytracking_amd.optimizer
  ltr.external.PreciseRoIPooling.pytorch.prroi_pool.PrRoIPool2D  (module is CREATED: the submodule is empty)
                                                                                      -> pytracking_amd.prroi_pool
  pytracking.libs.optimization.ConjugateGradient  (ConvProblem + MLU fast path)       -> pytracking_amd.optimization
  pytracking.libs.optimization.GaussNewtonCG      (FactorizedConvProblem fast path)   -> pytracking_amd.optimization
  pytracking.libs.operation.conv2d                (mode='same', one output channel: ATOM's per-frame classification)
                                                                                      -> pytracking_amd.filter.corr_raw
  pytracking.features.preprocessing.sample_patch / sample_patch_multiscale (device images)
                                                                                      -> pytracking_amd.preprocessing
  ltr.models.lwl.loss_residual_modules.LWTLResidual, ltr.models.meta.steepestdescent.GNSteepestDescent
                                                  (LWL few-shot learner)              -> pytracking_amd.steepestdescent
  ltr.models.meta.steepestdescent.GNSteepestDescent on residual_modules.LinearFilterHinge
                                                  (DiMP-simple, RTS classifier)       -> pytracking_amd.gn_hinge
  ltr.models.rts.loss_residual_modules.RTSResidual (RTS segmentation learner)         -> pytracking_amd.steepestdescent
  ltr.models.transformer.transformer.Transformer, ltr.models.transformer.filter_predictor.FilterPredictor,
  ltr.models.transformer.heads.{LinearFilterClassifier, DenseBoxRegressor}
                                                  (ToMP model predictor, inference)   -> pytracking_amd.transformer
  ltr.models.target_classifier.features.residual_bottleneck  (final 3x3 conv + InstanceL2Norm, inference)
                                                                                      -> pytracking_amd.features
  ltr.data.processing_utils.find_local_maxima, ltr.models.target_candidate_matching.target_candidate_matching
  .DescriptorExtractor.get_descriptors, ltr.models.target_candidate_matching.superglue.SuperGlue._forward
                                                  (KeepTrack candidate matching)      -> pytracking_amd.candidate_matching
  spatial_correlation_sampler  (module is CREATED when nothing importable is there: a CUDA extension without a ROCm build),
  ltr.models.kys.predictor_wrapper.PredictorWrapper.predict_response, ltr.models.kys.cost_volume.CostVolume.forward
                                                  (KYS response prediction)           -> pytracking_amd.kys
  pytracking.libs.dcf.max2d, pytracking.tracker.dimp.dimp.DiMP.localize_advanced (and DiMPSimple's, KeepTrack's),
  pytracking.tracker.tomp.tomp.ToMP.localize_advanced  (score-map localisation)       -> pytracking_amd.localization
  pytracking.tracker.dimp.dimp.DiMP.optimize_boxes_default / optimize_boxes_relative (and DiMPSimple's, KeepTrack's),
  pytracking.tracker.atom.atom.ATOM.optimize_boxes                                    (IoU-guided box refinement)
                                                                                      -> pytracking_amd.iou_refine
  ltr.models.target_classifier.features.residual_basic_block, and residual_bottleneck with final_stride=2
                                                  (LWL / RTS target-model head, RTS classifier head; only with
                                                  install(feature_heads=True))        -> pytracking_amd.features
  ltr.models.bbreg.atom_iou_net.AtomIoUNet.get_iou_feat  (both IoU feature towers; only with install(iou_feat=True))
                                                                                      -> pytracking_amd.iou_feat
  ltr.models.bbreg.atom_iou_net.AtomIoUNet.get_modulation  (the first frame's IoU modulation vectors; only with install(iou_mod=True))
                                                                                      -> pytracking_amd.iou_mod
  ltr.models.lwl.label_encoder.ResidualDS16SW.forward, ltr.models.rts.label_encoder.ResidualDS16SW.forward
                                                  (mask label encoder; only with install(label_encoder=True))
                                                                                      -> pytracking_amd.label_encoder
  ltr.models.{lwl,rts}.label_encoder.ResidualDS16FeatSWBox.forward, ...ResidualDS16FeatSWBoxCatMultiBlock.forward
                                                  (box label encoders of the first frame; only with install(box_encoder=True))
                                                                                      -> pytracking_amd.box_encoder
  ltr.models.lwl.decoder.LWTLDecoder.forward, ltr.models.rts.decoder.RTSDecoder.forward
                                                  (segmentation decoder, decoder.py:130-160; only with install(decoder=True))
                                                                                      -> pytracking_amd.lwl_decoder
  ltr.models.rts.label_encoder.ResidualDS16SW_Clf.forward, ltr.models.rts.rts_net.RTSNet.segment_target
                                                  (RTS instance-score encoder; resize + LearnersFusion between the target model and
                                                  the decoder; only with install(rts_fusion=True))
                                                                                      -> pytracking_amd.rts_fusion
  pytracking.tracker.lwl.lwl.LWL.convert_scores_crop_to_image / merge_results,
  pytracking.tracker.rts.sta_helper.STAHelper.convert_scores_crop_to_image,
  pytracking.tracker.rts.rts.RTS.convert_seg_scores_crop_to_image / merge_results
                                                  (crop-to-image paste and multi-object merge; only with install(seg_readout=True))
                                                                                      -> pytracking_amd.seg_readout

  pytracking.libs.fourier.cfft2 / cifft2 / shift_fs, pytracking.libs.dcf.get_reg_filter (the Fourier tools on torch.fft: the reference's
  call the removed torch.rfft / torch.irfft), pytracking.tracker.eco.eco.ECO.preprocess_sample / extract_fourier_sample / apply_filter /
  localize_target / update_memory, pytracking.tracker.eco.optim.FilterOptim.run
                                             (ECO's per-frame Fourier-domain path and filter update; only with install(eco=True))
                                                                                      -> pytracking_amd.eco
  pytracking.tracker.eco.eco.GaussNewtonCG   (the name eco.py:9 imported: ECO's first-frame joint Gauss-Newton optimisation of filter and
                                             projection matrix; only with install(eco_init=True), meant to go with eco=True)
                                                                                      -> pytracking_amd.eco
  ltr.models.transformer.filter_predictor.GOTFilterPredictor
                                             (TaMOs multi-object filter predictor, inference; only with install(tamos=True))
                                                                                      -> pytracking_amd.tamos
  ltr.models.transformer.heads.FPN, ltr.models.transformer.heads.DenseBoxRegressor
                                             (TaMOs two-level FPN and multi-object box regressor; only with install(tamos=True))
                                                                                      -> pytracking_amd.tamos
  pytracking.tracker.tamos.tamos.TaMOs.classify_target / localize_target / direct_bbox_regression / encode_bbox / get_label_function
                                             (TaMOs per-frame multi-object read-out and training targets, libpt_mot.so; only with
                                             install(tamos_readout=True), meant to go with tamos=True)
                                                                                      -> pytracking_amd.tamos_readout
  pytracking.tracker.atom.atom.ATOM.localize_target
                                             (ATOM's per-frame score localisation: Fourier upsampling, window, both peaks and the
                                             outcome, libpt_loc.so; only with install(atom_localize=True))
                                                                                      -> pytracking_amd.atom_localize
  pytracking.tracker.{dimp.dimp.DiMP, kys.kys.KYS, tomp.tomp.ToMP, dimp_simple.dimp_simple.DiMPSimple, tamos.tamos.TaMOs,
  keep_track.keep_track.KeepTrack, atom.atom.ATOM, lwl.lwl.LWL, rts.rts.RTS}.update_memory
                                             (the per-frame sample-memory update: weight decay, slot arg-min, floor and the stores of
                                             the sample, label, box and mask, libpt_mem.so; only with install(memory=True))
                                                                                      -> pytracking_amd.memory_update
  ltr.models.backbone.resnet.ResNet.forward, ltr.models.backbone.resnet_mrcnn.ResNet.forward
                                             (the ResNet backbone forward: stem, pool and residual blocks up to the deepest requested
                                             layer, libpt_bbn.so; only with install(backbone=True))
                                                                                      -> pytracking_amd.backbone

Dispatch rule of the rebound *functions*: device fp32 tensors of a shape the gfx950 kernels cover go to the C ABI;
everything else (CPU tensors, dilations, grouped filters, K*K > 16, more than 16 filters) is outside the hot path and
is handed to the reference's ORIGINAL function object -- its own stock-PyTorch code, not a re-implementation --
unless `strict=True`, in which case it raises (`_outside` is the one place that decides).  The rebound optimiser /
learner *classes* follow the same rule per call of their `forward`; the classes that choose an implementation when they
are constructed (`Transformer`, `LWTLResidual`, `ConjugateGradient` ...) follow it per construction.

Every rebinding -- module attributes, class attributes, names other modules imported by value, `sys.modules` entries --
goes through `_rebind` / `_rebind_module`, which record `(owner, name, previous binding or _MISSING, new binding)` in one
ordered ledger.  `uninstall()` replays the ledger backwards (set the previous binding, delete what did not exist) and has
no per-family knowledge; an `install()` that raises replays what it had recorded, so nothing stays half installed.
`installed()` and `original(owner, name)` are the public view of that state.
"""
import collections
import functools
import importlib
import sys
import types

import torch

from . import filter as _filter
from . import optimization as _optimization
from . import optimizer as _optimizer
from . import prroi_pool as _prroi
from . import steepestdescent as _sd

_MISSING = object()
_state = {"installed": False, "strict": False, "ledger": []}

# which branch every rebound symbol took, per call: "<symbol>.fast" (gfx950 path) / "<symbol>.reference" (handed to the
# reference's own code).  tests/test_trackers_on_device.py asserts on it that a tracker running on the GPU really went
# through the HIP library; reset with `stats.clear()`.
stats = collections.Counter()


def installed():
    """True from a successful `install()` to the next `uninstall()`."""
    return _state["installed"]


def original(owner, name):
    """The object `owner.name` was bound to before install() rebound it: the reference's own function, method or class."""
    for o, n, prev, _ in _state["ledger"]:
        if o is owner and n == name and prev is not _MISSING:
            return prev
    raise KeyError(f"{name}: not rebound by install()")


def _rebind(owner, name, value):
    """`owner.name = value` (module or class), recorded in the ledger."""
    _state["ledger"].append((owner, name, vars(owner).get(name, _MISSING), value))
    setattr(owner, name, value)


def _rebind_module(name, module):
    """`sys.modules[name] = module`, recorded in the ledger."""
    _state["ledger"].append((sys.modules, name, sys.modules.get(name, _MISSING), module))
    sys.modules[name] = module


def _replay(keep=0):
    """Undo the ledger's entries beyond the first `keep`, last first."""
    ledger = _state["ledger"]
    while len(ledger) > keep:
        owner, name, prev, new = ledger.pop()
        if owner is not sys.modules:
            if prev is _MISSING:
                delattr(owner, name)
            else:
                setattr(owner, name, prev)
        elif prev is not _MISSING:
            sys.modules[name] = prev
        elif sys.modules.get(name) is new:                   # an entry we created: removed only while it is still ours
            del sys.modules[name]


def _hit(name, fast):
    stats[name + (".fast" if fast else ".reference")] += 1
    return fast


def _outside(message):
    """A call or configuration outside the gfx950 hot path: raises under `install(strict=True)`; otherwise returns, and the caller
    hands the call to the reference's own code."""
    if _state["strict"]:
        raise NotImplementedError(message)


def _dispatcher(ref, name, covered, fast, message):
    """The function bound in place of `ref` (a function, a method, or the `forward` of a dispatching class): calls that `covered`
    accepts go to `fast`, the others to `ref` (or raise under strict).  `covered` and `fast` take the reference's arguments."""
    hit, miss = name + ".fast", name + ".reference"

    def wrapper(*args, **kw):
        if covered(*args, **kw):
            stats[hit] += 1
            return fast(*args, **kw)
        stats[miss] += 1
        _outside(message)
        return ref(*args, **kw)

    wrapper.__name__, wrapper.__doc__, wrapper.__wrapped__ = ref.__name__, ref.__doc__, ref
    return wrapper


def _choosing_class(ref, covered, ours, message=None, doc=None):
    """The class bound under the name of the reference class `ref`: constructor arguments that `covered` accepts build `ours`
    (the gfx950 module), the others the reference class (or raise under strict, when there is a `message`).  It subclasses `ref`,
    so the reference's own `isinstance` / `issubclass` checks keep working."""
    class Choosing(ref):
        __doc__ = doc

        def __new__(cls, *args, **kw):
            if covered(*args, **kw):
                return ours(*args, **kw)
            if message:
                _outside(message)
            return ref.__new__(cls)

    Choosing.__name__ = Choosing.__qualname__ = ref.__name__
    Choosing._pt_reference = ref
    return Choosing


def _covered(feat, filt, dilation_factors=None):
    if not (isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32 and filt.is_cuda
            and dilation_factors is None):
        return False
    if torch.is_grad_enabled() and feat.requires_grad:   # feature gradients (offline training): the reference's convs
        return False
    if filt.dim() == 5:                                  # multi-filter (LWL): <= 16 filters, 1x1 / 3x3, groups == 1
        return (filt.shape[1] <= 16 and filt.shape[-1] == filt.shape[-2] and filt.shape[-1] in (1, 3)
                and filt.shape[-3] == feat.shape[-3] and feat.shape[-1] <= 256)
    return filt.dim() == 4 and filt.shape[-1] * filt.shape[-2] <= 16


def _install_filter_layer():
    """`apply_filter` / `apply_feat_transpose` / `filter_gradient`: modules that did `import ltr.models.layers.filter as filter_layer`
    see the rebinding through the module object; nothing in the hot path does `from ... import apply_filter`."""
    fmod = importlib.import_module("ltr.models.layers.filter")

    def covered_transpose(feat, input, filter_ksz, training=True, groups=1):
        ksz = (filter_ksz, filter_ksz) if isinstance(filter_ksz, int) else tuple(filter_ksz)
        mf = input.dim() == 5 and input.shape[2] <= 16 and ksz[0] == ksz[1] and ksz[0] in (1, 3) and feat.shape[-1] <= 256
        return (feat.is_cuda and feat.dtype == torch.float32 and groups == 1
                and (mf or (input.dim() == 4 and ksz[0] * ksz[1] <= 16))
                and not (torch.is_grad_enabled() and feat.requires_grad))

    for name, covered in (("apply_filter", _covered), ("apply_feat_transpose", covered_transpose),
                          ("filter_gradient", lambda feat, filter, label=None, training=True: _covered(feat, filter))):
        _rebind(fmod, name, _dispatcher(getattr(fmod, name), name, covered, getattr(_filter, name),
                                        name + ": configuration outside the gfx950 hot path"))


def _optimizer_class(fused_cls, ref_cls):
    """The class bound under the reference's name: the gfx950 module (same parameters, same state_dict keys) whose
    forward runs the fused solver for device tensors under no_grad and hands every other call (CPU tensors, offline
    training with requires_grad inputs, K*K > 16) to the reference class's own forward on the same parameters."""
    import ltr.models.layers.activation as ract
    import ltr.models.layers.distance as rdist

    def covered(self, weights, feat, bb, sample_weight=None, num_iter=None, compute_losses=True):
        return (feat.is_cuda and weights.is_cuda and feat.dtype == torch.float32
                and weights.shape[-1] == weights.shape[-2] and weights.shape[-1] ** 2 <= 16
                and (sample_weight is None or isinstance(sample_weight, torch.Tensor))
                and not (torch.is_grad_enabled() and (weights.requires_grad or feat.requires_grad)))

    class Dispatching(fused_cls):
        __doc__ = ref_cls.__doc__

        def __init__(self, *args, **kw):
            super().__init__(*args, **kw)
            # parameter-free helper modules the reference forward reads (optimizer.py:44,74-82)
            if hasattr(self, "num_dist_bins"):
                self.distance_map = rdist.DistanceMap(self.num_dist_bins, self.bin_displacement)
                if self.score_act == 'bentpar':
                    self.score_activation = ract.BentIdentPar(self.act_param)
                    self.score_activation_deriv = ract.BentIdentParDeriv(self.act_param)
                else:
                    self.score_activation = ract.LeakyReluPar()
                    self.score_activation_deriv = ract.LeakyReluParDeriv()

        forward = _dispatcher(ref_cls.forward, ref_cls.__name__, covered, fused_cls.forward,
                              f"{ref_cls.__name__}: call outside the gfx950 hot path")

    for name, member in vars(ref_cls).items():           # helper methods the reference forward calls (get_label_density ...)
        if callable(member) and not name.startswith("__") and not hasattr(fused_cls, name):
            setattr(Dispatching, name, member)
    Dispatching.__name__ = Dispatching.__qualname__ = ref_cls.__name__
    return Dispatching


def _install_optimizer_classes():
    omod = importlib.import_module("ltr.models.target_classifier.optimizer")
    for n in ("DiMPSteepestDescentGN", "DiMPL2SteepestDescentGN", "PrDiMPSteepestDescentNewton"):
        _rebind(omod, n, _optimizer_class(getattr(_optimizer, n), getattr(omod, n)))


def provide_prroi_module():
    """Create `ltr.external.PreciseRoIPooling.pytorch.prroi_pool` (an empty git submodule in the reference) in
    sys.modules so that `from ltr.external.PreciseRoIPooling.pytorch.prroi_pool import PrRoIPool2D`
    (initializer.py:4, atom_iou_net.py:4) resolves to the HIP implementation.  If an implementation was already
    registered under that name (a CPU stand-in in a test harness), CPU tensors keep going to it; modules that imported
    the class by name before this call are re-pointed.  `uninstall()` undoes it."""
    for pkg in ("ltr.external", "ltr.external.PreciseRoIPooling", "ltr.external.PreciseRoIPooling.pytorch"):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = []
            _rebind_module(pkg, m)
    name = "ltr.external.PreciseRoIPooling.pytorch.prroi_pool"
    prev_cls = getattr(sys.modules.get(name), "PrRoIPool2D", None)

    class PrRoIPool2D(_prroi.PrRoIPool2D):
        __doc__ = _prroi.PrRoIPool2D.__doc__

        def forward(self, features, rois):
            if _hit("PrRoIPool2D", features.is_cuda or prev_cls is None):
                return _prroi.PrRoIPool2D.forward(self, features, rois)
            return prev_cls(self.pooled_height, self.pooled_width, self.spatial_scale)(features, rois)

    pm = types.ModuleType(name)
    pm.PrRoIPool2D = PrRoIPool2D
    pm.prroi_pool2d = _prroi.prroi_pool2d
    _rebind_module(name, pm)
    _rebind(sys.modules["ltr.external.PreciseRoIPooling.pytorch"], "prroi_pool", pm)
    if prev_cls is not None:
        for modname in ("ltr.models.target_classifier.initializer", "ltr.models.bbreg.atom_iou_net"):
            mod = sys.modules.get(modname)
            if mod is not None and getattr(mod, "PrRoIPool2D", None) is prev_cls:
                _rebind(mod, "PrRoIPool2D", PrRoIPool2D)
    return pm


def _install_tomp():
    """ToMP model predictor (inference): the reference's tompnet constructors (ltr/models/tracking/tompnet.py:106-118)
    reach these classes through module attributes, so rebinding the attributes is enough."""
    from . import transformer as _tm
    try:
        tmod = importlib.import_module("ltr.models.transformer.transformer")
        pmod = importlib.import_module("ltr.models.transformer.filter_predictor")
        hmod = importlib.import_module("ltr.models.transformer.heads")
    except Exception:                   # torchvision (heads.py:3) missing: leave the transformer family alone
        return

    def covered(d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, dim_feedforward=2048, dropout=0.1,
                activation="relu", normalize_before=False, return_intermediate_dec=False):
        hd = d_model // max(nhead, 1)
        return (activation == "relu" and not normalize_before and not return_intermediate_dec and d_model % 128 == 0
                and d_model <= 512 and d_model % nhead == 0 and hd in (16, 32, 64) and nhead <= 16
                and dim_feedforward % 64 == 0 and num_encoder_layers <= 16 and num_decoder_layers <= 16)

    _rebind(tmod, "Transformer", _choosing_class(
        tmod.Transformer, covered, _tm.Transformer, "Transformer: configuration outside the gfx950 hot path",
        doc="Covered configuration -> gfx950 parameter container; anything else -> the reference class."))
    _rebind(pmod, "FilterPredictor", _choosing_class(
        pmod.FilterPredictor, lambda transformer, *args, **kw: isinstance(transformer, _tm.Transformer), _tm.FilterPredictor,
        "FilterPredictor: transformer outside the gfx950 hot path"))
    _rebind(hmod, "LinearFilterClassifier", _tm.LinearFilterClassifier)
    _rebind(hmod, "DenseBoxRegressor", _choosing_class(
        hmod.DenseBoxRegressor, lambda num_channels, *args, **kw: num_channels % 64 == 0 and num_channels <= 512,
        _tm.DenseBoxRegressor, "DenseBoxRegressor: channel count outside the gfx950 hot path"))


def _install_tamos():
    """TaMOs multi-object filter predictor, FPN and box regressor (inference): `tamosnet_resnet50` / `tamosnet_swin_base` (ltr/models/tracking/tamosnet.py) reach
    `GOTFilterPredictor` through the module attribute.  The gfx950 class is chosen for the gfx950 transformer container with
    label_enc 'gaussian', box_enc 'ltrb_token' and 1 <= num_tokens <= 16; anything else builds the reference class."""
    from . import tamos as _ta
    try:
        pmod = importlib.import_module("ltr.models.transformer.filter_predictor")
    except Exception:
        return
    _rebind(pmod, "GOTFilterPredictor", _choosing_class(
        pmod.GOTFilterPredictor, _ta.covered, _ta.GOTFilterPredictor,
        "GOTFilterPredictor: configuration outside the gfx950 hot path",
        doc="Covered configuration -> gfx950 multi-object predictor; anything else -> the reference class."))
    # the heads behind the predictor (tamos.py:308-317): heads.FPN and the DenseBoxRegressor that also takes T filters per sequence
    try:
        hmod = importlib.import_module("ltr.models.transformer.heads")
    except Exception:                   # torchvision (heads.py:3) missing: leave the heads alone
        return
    ref_reg = hmod.DenseBoxRegressor
    while "_pt_reference" in vars(ref_reg):                 # the default install()'s choosing class stands there already
        ref_reg = ref_reg._pt_reference
    _rebind(hmod, "DenseBoxRegressor", _choosing_class(
        ref_reg, _ta.regressor_covered, _ta.DenseBoxRegressor, "DenseBoxRegressor: channel count outside the gfx950 hot path"))

    def fpn_covered(high_res_layer="layer2", output_dim=256, input_dims=(512, 256)):
        dims = tuple(input_dims)
        return (len(dims) == 2 and all(isinstance(c, int) and c % 64 == 0 and 0 < c <= 2048 for c in dims)
                and isinstance(output_dim, int) and output_dim % 64 == 0 and 0 < output_dim <= 512)

    _rebind(hmod, "FPN", _choosing_class(hmod.FPN, fpn_covered, _ta.FPN, "FPN: configuration outside the gfx950 hot path"))


def _install_tamos_readout():
    """TaMOs per-frame multi-object read-out (`pytracking.tracker.tamos.tamos.TaMOs`, only with install(tamos_readout=True)): five methods of
    the unmodified class.  `classify_target` runs the reference method and queues ONE read-out launch for all active objects on its two
    outputs; `localize_target` and `direct_bbox_regression` answer from that stash after the frame's one wait; `encode_bbox` and
    `get_label_function` build the training targets on the device.  Every call the stash does not cover goes to the reference method."""
    from . import tamos_readout as _tr
    try:
        tmod = importlib.import_module("pytracking.tracker.tamos.tamos")
        TensorList = importlib.import_module("pytracking.libs.tensorlist").TensorList
    except Exception:                   # pytracking side not importable (missing cv2 ...)
        return
    cls = tmod.TaMOs
    for name, make in (("classify_target", _tr.make_classify_target), ("localize_target", _tr.make_localize_target),
                       ("direct_bbox_regression", _tr.make_direct_bbox_regression), ("encode_bbox", _tr.make_encode_bbox),
                       ("get_label_function", functools.partial(_tr.make_get_label_function, TensorList=TensorList))):
        ref = vars(cls)[name]
        covered, fast = make(ref)
        _rebind(cls, name, _dispatcher(ref, "TaMOs." + name, covered, fast, f"TaMOs.{name}: call outside the gfx950 read-out"))


def _install_atom_localize():
    """ATOM's per-frame score localisation (`pytracking.tracker.atom.atom.ATOM.localize_target`, atom.py:304-406; only with
    install(atom_localize=True)): the Fourier interpolation onto the output grid, the output window, both peaks and every outcome of
    `localize_advanced` in two launches and one wait.  `scale_ind` comes back as a CPU tensor, which atom.py:252 needs under torch 2.  CPU or
    non-float32 scores, more than one feature block, `debug >= 2` and sizes outside include/pt_loc.h go to the reference method -- which
    calls torch.rfft / torch.irfft and therefore works only next to `install(eco=True)`'s Fourier tools.  Off by default: the set a default
    install() rebinds is pinned."""
    from . import atom_localize as _al
    try:
        cls = importlib.import_module("pytracking.tracker.atom.atom").ATOM
    except Exception:                   # pytracking side not importable (missing cv2 ...)
        return
    ref = vars(cls)["localize_target"]
    _rebind(cls, "localize_target", _dispatcher(ref, "ATOM.localize_target", _al.covered_localize_target, _al.tracker_localize_target,
                                                "ATOM.localize_target: call outside the gfx950 localisation"))


def _install_memory():
    """The per-frame sample-memory update (`update_memory` of DiMP, KYS, ToMP, DiMPSimple, TaMOs, KeepTrack, ATOM, LWL and RTS; only with
    install(memory=True)): the weight decay, the arg-min of the slot, the renormalisation, the `init_samples_minimum_weight` floor and the
    stores of the sample and its label / box / mask in two launches of libpt_mem.so, without a host wait while the memory fills and with
    one behind it.  A tracker on the CPU, memories that are not contiguous float32, sizes outside include/pt_mem.h and a source that overlaps
    its memory go to the reference method.  The `update_sample_weights*` methods stay the reference's (`init_memory` calls them).  Off by
    default: the set a default install() rebinds is pinned."""
    from . import memory_update as _mu
    for name, entry in _mu.TABLE.items():
        try:
            cls = getattr(importlib.import_module(entry.module), name)
        except Exception:               # pytracking side not importable (missing cv2 ...)
            continue
        ref = vars(cls)["update_memory"]
        covered, fast = _mu.make(name)
        _rebind(cls, "update_memory", _dispatcher(ref, name + ".update_memory", covered, fast,
                                                  f"{name}.update_memory: call outside the gfx950 memory update"))


def _install_backbone():
    """The ResNet backbone forward (`ResNet.forward` of ltr/models/backbone/resnet.py and resnet_mrcnn.py; only with
    install(backbone=True)): the stem, the max-pool and the residual blocks up to the deepest requested layer in libpt_bbn.so.  CPU,
    non-fp32 or non-contiguous input, training mode or enabled gradients, dilated networks, BasicBlock(use_bn=False), a request for `fc` /
    'default' or an unknown layer and sizes outside include/pt_bbn.h go to the reference method.  Both classes count as `ResNet.forward`.
    Off by default: the set a default install() rebinds is pinned."""
    from . import backbone as _bb
    for modname in ("ltr.models.backbone.resnet", "ltr.models.backbone.resnet_mrcnn"):
        try:
            cls = importlib.import_module(modname).ResNet
        except Exception:               # ltr side not importable
            continue
        _rebind(cls, "forward", _dispatcher(vars(cls)["forward"], "ResNet.forward", _bb.covered, functools.partial(_bb.forward, checked=True),
                                            "ResNet.forward: call outside the gfx950 backbone"))


def _install_clf_head(feature_heads=False):
    """Classification-feature head: `clf_features.residual_bottleneck(...)` is reached through the module attribute by
    every network constructor (dimpnet.py:169, tompnet.py:99).  Covered argument sets build the fused module around the
    reference's own layer objects; on a CPU tensor / in training it runs those layers as `nn.Sequential` would.
    `feature_heads` (off unless `install(feature_heads=True)`: the set a default install() rebinds is pinned): the rebound
    `residual_bottleneck` also takes `final_stride=2` (RTS classifier head, rts_net.py:339-344) and `residual_basic_block`
    (LWL / RTS target-model head, lwl_net.py:173-177, rts_net.py:294-298) is rebound the same way."""
    from . import features as _fm
    try:
        fmod = importlib.import_module("ltr.models.target_classifier.features")
    except Exception:                   # torchvision (features.py:4) missing
        return
    ref_fn = fmod.residual_bottleneck

    def fused(self, x):
        return (x.is_cuda and x.dtype == torch.float32 and not self.training
                and not (torch.is_grad_enabled() and (x.requires_grad or self[0].weight.requires_grad)))

    class ClfHead(_fm.ClfHead):
        forward = _dispatcher(torch.nn.Sequential.forward, "residual_bottleneck", fused, _fm.ClfHead.forward,
                              "clf feature head: call outside the gfx950 hot path")

    covered = _fm.covered_strided if feature_heads else _fm.covered

    def residual_bottleneck(*args, **kw):
        seq = ref_fn(*args, **kw)
        if covered(*args, **kw) and len(seq) == 2:
            return ClfHead(seq[0], seq[1])                # the reference's Conv2d and InstanceL2Norm objects
        _outside("residual_bottleneck: configuration outside the gfx950 hot path")
        return seq

    residual_bottleneck.__doc__ = ref_fn.__doc__
    residual_bottleneck.__wrapped__ = ref_fn
    _rebind(fmod, "residual_bottleneck", residual_bottleneck)
    if not feature_heads:
        return
    ref_bb = fmod.residual_basic_block

    class FeatHead(_fm.ClfHead):
        forward = _dispatcher(torch.nn.Sequential.forward, "residual_basic_block", fused, _fm.ClfHead.forward,
                              "feature head: call outside the gfx950 hot path")

    def residual_basic_block(*args, **kw):
        seq = ref_bb(*args, **kw)
        if _fm.covered_basic_block(*args, **kw) and len(seq) == 2:
            return FeatHead(seq[0], seq[1])               # the reference's Conv2d and InstanceL2Norm objects
        _outside("residual_basic_block: configuration outside the gfx950 hot path")
        return seq

    residual_basic_block.__doc__ = ref_bb.__doc__
    residual_basic_block.__wrapped__ = ref_bb
    _rebind(fmod, "residual_basic_block", residual_basic_block)


def _install_localization():
    """`dcf.max2d` (function, reached as `dcf.max2d` by the trackers) and the `localize_advanced` methods of DiMP / ToMP:
    one launch + one 32-byte copy per frame instead of ~10 host synchronisations."""
    from . import localization as _loc
    try:
        dmod = importlib.import_module("pytracking.libs.dcf")
    except Exception:
        return
    _rebind(dmod, "max2d", _dispatcher(dmod.max2d, "max2d", lambda a: a.is_cuda and a.dtype == torch.float32, _loc.max2d,
                                       "max2d: tensor outside the gfx950 hot path"))

    def covered(self, scores, sample_pos, sample_scales):
        return scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 3 and scores.shape[0] <= 8

    for modname, clsname, fast in (("pytracking.tracker.dimp.dimp", "DiMP", _loc.localize_advanced),
                                   ("pytracking.tracker.dimp_simple.dimp_simple", "DiMPSimple", _loc.localize_advanced),   # = DiMP's
                                   ("pytracking.tracker.keep_track.keep_track", "KeepTrack", _loc.localize_advanced),      # = DiMP's
                                   ("pytracking.tracker.tomp.tomp", "ToMP", _loc.localize_advanced_tomp)):
        try:
            cls = getattr(importlib.import_module(modname), clsname)
        except Exception:               # tracker module not importable here (cv2 ...): nothing to patch
            continue
        _rebind(cls, "localize_advanced", _dispatcher(cls.localize_advanced, clsname + ".localize_advanced", covered, fast,
                                                      "localize_advanced: scores outside the gfx950 hot path"))


def _install_iou_refine():
    """`DiMP.optimize_boxes_default` / `optimize_boxes_relative` (dimp.py:725-788): all refinement iterations in one
    device-side sequence instead of one autograd graph per iteration."""
    from . import iou_refine as _ir
    try:
        cls = importlib.import_module("pytracking.tracker.dimp.dimp").DiMP
    except Exception:
        return
    both = (("optimize_boxes_default", _ir.optimize_boxes_default), ("optimize_boxes_relative", _ir.optimize_boxes_relative))
    targets = [(cls, name, fast, lambda t: t.net.bb_regressor) for name, fast in both]
    # DiMPSimple's two methods are DiMP's, byte for byte (dimp_simple.py vs dimp.py); KeepTrack's differ from DiMP's in comments and
    # docstrings only (keep_track.py vs dimp.py)
    for modname, clsname in (("pytracking.tracker.dimp_simple.dimp_simple", "DiMPSimple"),
                             ("pytracking.tracker.keep_track.keep_track", "KeepTrack")):
        try:
            scls = getattr(importlib.import_module(modname), clsname)
        except Exception:
            continue
        targets += [(scls, name, fast, lambda t: t.net.bb_regressor) for name, fast in both]
    try:
        acls = importlib.import_module("pytracking.tracker.atom.atom").ATOM
        targets.append((acls, "optimize_boxes", _ir.optimize_boxes_atom, lambda t: t.iou_predictor))
    except Exception:
        pass
    for cls, name, fast, get_net in targets:
        ref_method = getattr(cls, name)

        def method(self, iou_features, init_boxes, _fast=fast, _ref=ref_method, _net=get_net,
                   _name=cls.__name__ + "." + name):
            feats = list(iou_features)
            ok = (len(feats) == 2 and all(f.is_cuda and f.dtype == torch.float32 and f.shape[0] == 1 for f in feats)
                  and not _net(self).training)
            if ok:
                try:
                    out = _fast(self, feats, init_boxes)
                    _hit(_name, True)
                    return out
                except NotImplementedError as exc:
                    _outside(str(exc))
            _hit(_name, False)
            if not ok:
                _outside(f"{_ref.__name__}: call outside the gfx950 hot path")
            return _ref(self, iou_features, init_boxes)

        method.__doc__, method.__wrapped__ = ref_method.__doc__, ref_method
        _rebind(cls, name, method)


def _install_operation():
    """`pytracking.libs.operation.conv2d` (operation.py:6-33; TensorList-lifted): ATOM classifies every frame with
    `operation.conv2d(sample_x, self.filter, mode='same')` (atom.py:300-302).  A single-output-channel 'same'
    correlation on device tensors goes to the gfx950 correlation pass; every other use (full inner products of
    optim.py:58-99, 1x1 projections, autograd) keeps the reference's function."""
    try:
        omod = importlib.import_module("pytracking.libs.operation")
        tl = importlib.import_module("pytracking.libs.tensorlist")
    except Exception:
        return
    ref_conv2d = omod.conv2d
    ref_single = getattr(ref_conv2d, "__wrapped__", None)     # functools.wraps keeps the un-lifted function
    if ref_single is None:
        return

    def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, mode=None):
        fused = (weight is not None and mode == 'same' and bias is None and stride == 1 and dilation == 1 and groups == 1
                 and padding == 0 and isinstance(input, torch.Tensor) and input.is_cuda and input.dtype == torch.float32
                 and input.dim() == 4 and weight.dim() == 4 and weight.shape[0] == 1 and weight.shape[1] == input.shape[1]
                 and weight.shape[2] * weight.shape[3] <= 16 and weight.is_cuda
                 and not (torch.is_grad_enabled() and (input.requires_grad or weight.requires_grad)))
        same_on_device = mode == 'same' and isinstance(input, torch.Tensor) and input.is_cuda
        if same_on_device:                                    # the classification call; the 1x1 projection (mode None) is stock
            _hit("operation.conv2d[same]", fused)             # PyTorch by design
        if fused:
            return _filter.corr_raw(input, weight[0], out_hw=tuple(input.shape[-2:])).unsqueeze(1)
        if same_on_device:
            _outside("operation.conv2d(mode='same'): configuration outside the gfx950 hot path")
        return ref_single(input, weight, bias=bias, stride=stride, padding=padding, dilation=dilation, groups=groups,
                          mode=mode)

    conv2d.__doc__ = ref_single.__doc__
    lifted = tl.tensor_operation(conv2d)
    lifted.__wrapped_reference__ = ref_conv2d
    _rebind(omod, "conv2d", lifted)


def _install_preprocessing():
    """`sample_patch` / `sample_patch_multiscale` (pytracking/features/preprocessing.py:33-148): for an image tensor that
    lives on the device, crop + replicate padding + bilinear resize become one gather launch.  The reference trackers
    build the image with `numpy_to_torch` on the CPU, so this route is taken when the caller uploads the frame first;
    CPU images and masks keep the reference's functions (also under strict, which refuses device images only); the first-frame
    augmentation set (`sample_patch_transformed`) runs on the device for the transforms pytracking_amd/preprocessing.py covers and
    falls back to the reference for the rest."""
    from . import preprocessing as _pp
    try:
        pmod = importlib.import_module("pytracking.features.preprocessing")
    except Exception:
        return
    ref_sp, ref_ms, ref_tr = pmod.sample_patch, pmod.sample_patch_multiscale, pmod.sample_patch_transformed

    def sample_patch(im, pos, sample_sz, output_sz=None, mode='replicate', max_scale_change=None, is_mask=False):
        if _hit("sample_patch", im.is_cuda and im.dtype == torch.float32 and not is_mask and im.dim() == 4 and im.shape[0] == 1):
            return _pp.sample_patch(im, pos, sample_sz, output_sz, mode=mode, max_scale_change=max_scale_change)
        if im.is_cuda:
            _outside("sample_patch: call outside the gfx950 hot path")
        return ref_sp(im, pos, sample_sz, output_sz, mode=mode, max_scale_change=max_scale_change, is_mask=is_mask)

    def sample_patch_multiscale(im, pos, scales, image_sz, mode='replicate', max_scale_change=None):
        n = 1 if isinstance(scales, (int, float)) else len(scales)
        if _hit("sample_patch_multiscale", im.is_cuda and im.dtype == torch.float32 and im.dim() == 4 and im.shape[0] == 1 and n <= 8):
            return _pp.sample_patch_multiscale(im, pos, scales, image_sz, mode=mode, max_scale_change=max_scale_change)
        if im.is_cuda:
            _outside("sample_patch_multiscale: call outside the gfx950 hot path")
        return ref_ms(im, pos, scales, image_sz, mode=mode, max_scale_change=max_scale_change)

    def sample_patch_transformed(im, pos, scale, image_sz, transforms, is_mask=False):
        # first-frame augmentation set (generate_init_samples, dimp.py:329-395): one gather launch over the base patch
        if im.is_cuda and im.dtype == torch.float32 and not is_mask and im.dim() == 4 and im.shape[0] == 1:
            try:
                out = _pp.sample_patch_transformed(im, pos, scale, image_sz, transforms)
                _hit("sample_patch_transformed", True)
                return out
            except NotImplementedError as exc:                # a transform the device path does not cover (RandomAffine, ...)
                _outside(str(exc))
        elif im.is_cuda:
            _outside("sample_patch_transformed: call outside the gfx950 hot path")
        _hit("sample_patch_transformed", False)
        return ref_tr(im, pos, scale, image_sz, transforms, is_mask=is_mask)

    wrappers = (("sample_patch", sample_patch, ref_sp), ("sample_patch_multiscale", sample_patch_multiscale, ref_ms),
                ("sample_patch_transformed", sample_patch_transformed, ref_tr))
    for name, fn, ref in wrappers:
        fn.__doc__, fn.__wrapped__ = ref.__doc__, ref
        _rebind(pmod, name, fn)
    # the trackers import the names (`from pytracking.features.preprocessing import sample_patch_multiscale, ...`)
    # ... and ATOM reaches them through its feature extractors (`pytracking/features/extractor.py:3,112`)
    for modname in ("pytracking.tracker.dimp.dimp", "pytracking.tracker.dimp_simple.dimp_simple", "pytracking.tracker.keep_track.keep_track",
                    "pytracking.tracker.atom.atom", "pytracking.tracker.tomp.tomp",
                    "pytracking.tracker.kys.kys", "pytracking.tracker.lwl.lwl", "pytracking.features.extractor",
                    "pytracking.features.featurebase"):
        try:
            tmod = importlib.import_module(modname)
        except Exception:
            continue
        for name, fn, ref in wrappers:
            if getattr(tmod, name, None) is ref:
                _rebind(tmod, name, fn)


def _install_candidate_matching():
    """KeepTrack's target-candidate matching (keep_track.py:437-475): `ltr.data.processing_utils.find_local_maxima` (reached as
    `prutils.find_local_maxima`), `DescriptorExtractor.get_descriptors` and `SuperGlue._forward`.  CPU tensors, grad-enabled
    calls, training mode, the bottleneck / input-projection / double-softmax variants, more than 64 candidates on a side and the
    reference's zero-keypoint branch keep the reference's code."""
    from . import candidate_matching as _cm
    try:
        pmod = importlib.import_module("ltr.data.processing_utils")
        tmod = importlib.import_module("ltr.models.target_candidate_matching.target_candidate_matching")
        gmod = importlib.import_module("ltr.models.target_candidate_matching.superglue")
    except Exception:
        return
    for owner, attr, name, covered, fast in (
            (pmod, "find_local_maxima", "find_local_maxima", _cm.covered_find_local_maxima, _cm.find_local_maxima),
            (tmod.DescriptorExtractor, "get_descriptors", "DescriptorExtractor.get_descriptors", _cm.covered_get_descriptors,
             _cm.get_descriptors),
            (gmod.SuperGlue, "_forward", "SuperGlue._forward", _cm.covered_match, functools.partial(_cm.match, checked=True))):
        _rebind(owner, attr, _dispatcher(getattr(owner, attr), name, covered, fast, name + ": call outside the gfx950 hot path"))


def provide_correlation_sampler():
    """Register pytracking_amd.kys as `spatial_correlation_sampler` (the CUDA extension ltr/models/kys/cost_volume.py:5 imports; it has
    no ROCm build) when nothing importable is there, so that `import ltr.models.tracking.kysnet` works.  An installed package or a module
    somebody else registered under that name (a CPU stand-in in a test harness) is left alone.  `uninstall()` removes the entry this
    call created, and only while it is still this module."""
    import importlib.util
    name = "spatial_correlation_sampler"
    if name in sys.modules:
        return sys.modules[name]
    try:
        found = importlib.util.find_spec(name) is not None
    except (ImportError, ValueError):
        found = False
    if found:
        return None
    from . import kys as _kys
    _rebind_module(name, _kys)
    return _kys


def _install_kys():
    """KYS (kys.py:314): `PredictorWrapper.predict_response` and `CostVolume.forward`.  CPU tensors, grad-enabled calls, training mode, a
    list of reference frames, a structure off the covered list of include/pt_hot.h (covered: representation_predictor_dims (16,) with
    conf_measure 'entropy' / 'max' / 'none' -- the trained network -- and (64, 32) with 'max' / 'none') and maps above 20 x 20 keep the
    reference's code."""
    from . import kys as _kys
    provide_correlation_sampler()
    try:
        wmod = importlib.import_module("ltr.models.kys.predictor_wrapper")
        cmod = importlib.import_module("ltr.models.kys.cost_volume")
    except Exception:
        return

    def covered_cost_volume(self, feat1, feat2):
        assert feat1.dim() == 4 and feat2.dim() == 4, 'Expect 4 dimensional inputs'
        return _kys.covered_cost_volume(self, feat1, feat2)

    for cls, attr, name, covered, fast in (
            (wmod.PredictorWrapper, "predict_response", "PredictorWrapper.predict_response", _kys.covered_predict_response,
             functools.partial(_kys.predict_response, checked=True)),
            (cmod.CostVolume, "forward", "CostVolume.forward", covered_cost_volume, _kys.cost_volume_forward)):
        _rebind(cls, attr, _dispatcher(getattr(cls, attr), name, covered, fast, name + ": call outside the gfx950 hot path"))


def _install_iou_feat():
    """`AtomIoUNet.get_iou_feat` (atom_iou_net.py:172-179): both towers of two Conv2d + BatchNorm2d + ReLU blocks in one call.  CPU
    tensors, training mode, grad-enabled calls, blocks of another structure (dilation ...) and uncovered shapes keep the reference's code.
    Off unless `install(iou_feat=True)`: the set a default install() rebinds is pinned."""
    from . import iou_feat as _if
    try:
        cls = importlib.import_module("ltr.models.bbreg.atom_iou_net").AtomIoUNet
    except Exception:
        return
    name = "AtomIoUNet.get_iou_feat"
    _rebind(cls, "get_iou_feat", _dispatcher(cls.get_iou_feat, name, _if.covered, functools.partial(_if.get_iou_feat, checked=True),
                                             name + ": call outside the gfx950 hot path"))


def _install_iou_mod():
    """`AtomIoUNet.get_modulation` (atom_iou_net.py:138-170): conv3_1r / conv4_1r on the pixel window under each first-frame box, both
    poolings, fc3_1r and the two fc34 blocks in one call.  CPU tensors, training mode, grad-enabled calls (the training `forward` calls
    it under autograd), blocks or pooling objects of another structure, a `bb` that is not (n, 4) on the maps' device and uncovered
    shapes keep the reference's code.  Off unless `install(iou_mod=True)`: the set a default install() rebinds is pinned."""
    from . import iou_mod as _im
    try:
        cls = importlib.import_module("ltr.models.bbreg.atom_iou_net").AtomIoUNet
    except Exception:
        return
    name = "AtomIoUNet.get_modulation"
    _rebind(cls, "get_modulation", _dispatcher(cls.get_modulation, name, _im.covered, functools.partial(_im.get_modulation, checked=True),
                                               name + ": call outside the gfx950 hot path"))


def _install_label_encoder():
    """`ResidualDS16SW.forward` of LWL and of RTS (label_encoder.py:38-55, the same code in both packages): stem, two BasicBlocks and both
    heads in six launches.  CPU tensors, training mode, grad-enabled calls, modules of another structure and uncovered channel counts keep
    the reference's code.  Off unless `install(label_encoder=True)`: the set a default install() rebinds is pinned."""
    from . import label_encoder as _le
    name = "ResidualDS16SW.forward"
    for modname in ("ltr.models.lwl.label_encoder", "ltr.models.rts.label_encoder"):
        try:
            cls = importlib.import_module(modname).ResidualDS16SW
        except Exception:
            continue
        _rebind(cls, "forward", _dispatcher(cls.forward, name, _le.covered, functools.partial(_le.forward, checked=True),
                                            name + ": call outside the gfx950 hot path"))


def _install_box_encoder():
    """`ResidualDS16FeatSWBox.forward` and `ResidualDS16FeatSWBoxCatMultiBlock.forward` of LWL and of RTS (label_encoder.py:108-126 and
    :188-216, the same code in both packages): the box is rasterised on the device, the mask trunk or the resized mask plane and the
    blocks over feature + mask encoding run without a concatenated map.  CPU tensors, use_gauss=True, training mode, grad-enabled calls,
    a `bb` of the wrong rank, modules of another structure and uncovered dims keep the reference's code.  Off unless
    `install(box_encoder=True)`: the set a default install() rebinds is pinned."""
    from . import box_encoder as _be
    for modname in ("ltr.models.lwl.label_encoder", "ltr.models.rts.label_encoder"):
        for clsname in (_be.BOX, _be.CAT):
            try:
                cls = getattr(importlib.import_module(modname), clsname)
            except Exception:
                continue
            name = clsname + ".forward"
            _rebind(cls, "forward", _dispatcher(cls.forward, name, _be.covered, functools.partial(_be.forward, checked=True),
                                                name + ": call outside the gfx950 hot path"))


def _install_lwl_decoder():
    """`LWTLDecoder.forward` (ltr/models/lwl/decoder.py:130-160) and `RTSDecoder.forward` (ltr/models/rts/decoder.py, the same code): all
    levels (TSE, RRB, CAB, RRB) and the Upsampler in one asynchronous call.  CPU tensors, training mode, grad-enabled calls, multi-object
    calls (`num_objects`), modules of another structure and uncovered shapes keep the reference's code.  Off unless
    `install(decoder=True)`: the set a default install() rebinds is pinned."""
    from . import lwl_decoder as _dec
    for modname, clsname in (("ltr.models.lwl.decoder", "LWTLDecoder"), ("ltr.models.rts.decoder", "RTSDecoder")):
        try:
            cls = getattr(importlib.import_module(modname), clsname)
        except Exception:
            continue
        name = clsname + ".forward"
        _rebind(cls, "forward", _dispatcher(cls.forward, name, _dec.covered, functools.partial(_dec.forward, checked=True),
                                            name + ": call outside the gfx950 hot path"))


def _install_rts_fusion():
    """`ResidualDS16SW_Clf.forward` (ltr/models/rts/label_encoder.py:86-103): the stride-1 score encoder in six launches; and
    `RTSNet.segment_target` (ltr/models/rts/rts_net.py:219-236): the bilinear resize of the encoded scores and the LearnersFusion in one
    launch between `target_model.apply_target_model` and `decoder`, which are called as they are bound.  CPU tensors, training mode,
    grad-enabled calls, calls without encoded scores, more than one sequence, modules of another structure and uncovered sizes keep the
    reference's code.  Off unless `install(rts_fusion=True)`: the set a default install() rebinds is pinned."""
    from . import rts_fusion as _rf
    try:
        enc_cls = importlib.import_module("ltr.models.rts.label_encoder").ResidualDS16SW_Clf
        net_cls = importlib.import_module("ltr.models.rts.rts_net").RTSNet
    except Exception:
        return
    for cls, attr, covered, fast in ((enc_cls, "forward", _rf.encoder_covered, functools.partial(_rf.encode, checked=True)),
                                     (net_cls, "segment_target", _rf.segment_covered, functools.partial(_rf.segment_target, checked=True))):
        name = cls.__name__ + "." + attr
        _rebind(cls, attr, _dispatcher(getattr(cls, attr), name, covered, fast, name + ": call outside the gfx950 hot path"))


def _install_seg_readout():
    """The segmentation trackers' read-out: `convert_scores_crop_to_image` of LWL and of RTS's STAHelper, RTS's
    `convert_seg_scores_crop_to_image` (resize + paste on the device, the score image comes back as the CPU tensor the trackers expect) and
    both `merge_results` (one upload, the soft aggregation with its arg-max and per-object statistics on the device, one download; the
    same numpy dictionaries).  CPU score tensors, a window that misses the image (the reference raises there), uncovered sizes, more than
    16 objects and a tracker without a GPU keep the reference's code.  `get_target_state` is not rebound: the unmodified trackers only
    hand it CPU tensors.  Off unless `install(seg_readout=True)`: the set a default install() rebinds is pinned."""
    from . import seg_readout as _sr

    def covered_rts(self, segmentation_scores, im, sample_coords):
        pos, scale = _sr.sample_location(self, sample_coords)
        return _sr.convert_covered(segmentation_scores, im, scale.item(), (pos[0].item(), pos[1].item()))

    def covered(self, segmentation_scores, im, sample_scale, sample_pos):
        return _sr.convert_covered(segmentation_scores, im, float(sample_scale), (float(sample_pos[0]), float(sample_pos[1])))

    for modname, clsname, attr, cov, fast in (
            ("pytracking.tracker.lwl.lwl", "LWL", "convert_scores_crop_to_image", covered, _sr.convert_scores_crop_to_image),
            ("pytracking.tracker.rts.sta_helper", "STAHelper", "convert_scores_crop_to_image", covered, _sr.convert_scores_crop_to_image),
            ("pytracking.tracker.rts.rts", "RTS", "convert_seg_scores_crop_to_image", covered_rts, _sr.convert_seg_scores_crop_to_image),
            ("pytracking.tracker.lwl.lwl", "LWL", "merge_results", _sr.merge_covered, _sr.merge_results_lwl),
            ("pytracking.tracker.rts.rts", "RTS", "merge_results", _sr.merge_covered, _sr.merge_results_rts)):
        try:
            cls = getattr(importlib.import_module(modname), clsname)
        except Exception:               # tracker module not importable here: nothing to patch
            continue
        name = clsname + "." + attr
        _rebind(cls, attr, _dispatcher(getattr(cls, attr), name, cov, fast, name + ": call outside the gfx950 hot path"))


def _install_eco():
    """ECO (pytracking/tracker/eco/eco.py).  `fourier.cfft2`, `fourier.cifft2` and `dcf.get_reg_filter` call torch.rfft / torch.irfft, which
    the installed torch does not have: they are REPLACED by pytracking_amd.eco's forms on torch.fft (any device; there is no reference code
    to hand a call to), `cfft2` of a covered device tensor by the sample-transform kernel.  `fourier.shift_fs` and the ECO methods
    `preprocess_sample`, `extract_fourier_sample`, `apply_filter`, `localize_target`, `update_memory` are dispatchers: CPU tensors,
    grad-enabled calls, other dtypes, debug >= 3, the 'transcale' fusion, a score grid equal to or smaller than the series and uncovered
    shapes keep the reference's code; so does `FilterOptim.run` (the filter update: all blocks, the CG state carried on the device).  The first-frame joint Gauss-Newton (whose problem class `_install_atom_cg`'s
    dispatcher declines; `_install_eco_init` has its kernels) and `symmetrize_filter` stay the reference's.  Off unless `install(eco=True)`: the set a default install() rebinds
    is pinned."""
    from . import eco as _eco
    try:
        fmod = importlib.import_module("pytracking.libs.fourier")
        dmod = importlib.import_module("pytracking.libs.dcf")
        lift = importlib.import_module("pytracking.libs.tensorlist").tensor_operation
    except Exception:
        return

    def cfft2(a):
        if _hit("cfft2", _eco.covered_cfft2(a)):
            return _eco.cfft2_device(a)
        return _eco.cfft2(a)

    for owner, name, fn in ((fmod, "cfft2", lift(cfft2)), (fmod, "cifft2", lift(_eco.cifft2)), (dmod, "get_reg_filter", _eco.get_reg_filter)):
        _rebind(owner, name, fn)
    ref_shift = fmod.shift_fs
    _rebind(fmod, "shift_fs", lift(_dispatcher(getattr(ref_shift, "__wrapped__", ref_shift), "shift_fs", _eco.covered_shift_fs, _eco.shift_fs,
                                               "shift_fs: call outside the gfx950 hot path")))
    try:
        cls = importlib.import_module("pytracking.tracker.eco.eco").ECO
    except Exception:               # tracker module not importable here: the Fourier tools are still provided
        return
    for attr, covered, fast in (("preprocess_sample", _eco.covered_preprocess_sample, _eco.tracker_preprocess_sample),
                                ("extract_fourier_sample", _eco.covered_extract_fourier_sample, _eco.tracker_extract_fourier_sample),
                                ("apply_filter", _eco.covered_tracker_apply_filter, _eco.tracker_apply_filter),
                                ("localize_target", _eco.covered_localize_target, _eco.tracker_localize_target),
                                ("update_memory", _eco.covered_update_memory, _eco.tracker_update_memory)):
        name = "ECO." + attr
        _rebind(cls, attr, _dispatcher(getattr(cls, attr), name, covered, fast, name + ": call outside the gfx950 hot path"))
    ocls = importlib.import_module("pytracking.tracker.eco.optim").FilterOptim
    _rebind(ocls, "run", _dispatcher(ocls.run, "FilterOptim.run", _eco.covered_filter_run, _eco.tracker_filter_run,
                                     "FilterOptim.run: call outside the gfx950 hot path"))


def _install_eco_init():
    """ECO's first-frame joint optimisation (eco.py:152-158).  Exactly one name is rebound: `pytracking.tracker.eco.eco.GaussNewtonCG`, which
    eco.py:9 imported by value, to a subclass of the reference's class whose `run` takes the kernels (pytracking_amd.eco.joint_init) for an
    `eco.optim.FactorizedConvProblem` on device fp32 tensors with debug off and integer iteration counts; every other object or call runs
    the reference's `run` (or raises under strict).  `pytracking.libs.optimization.GaussNewtonCG` is not touched: ATOM's dispatcher goes on
    declining ECO's problem.  Counters: `ECO.GaussNewtonCG.run.fast` / `.reference`.  Off unless `install(eco_init=True)`."""
    from . import eco as _eco
    try:
        emod = importlib.import_module("pytracking.tracker.eco.eco")
        problem_cls = importlib.import_module("pytracking.tracker.eco.optim").FactorizedConvProblem
    except Exception:
        return
    bound = emod.GaussNewtonCG
    ref = getattr(bound, "_pt_reference", bound)              # under a default install() the name may hold ATOM's choosing class

    def on_run(fast):
        if not _hit("ECO.GaussNewtonCG.run", fast):
            _outside("ECO.GaussNewtonCG.run: call outside the gfx950 hot path")

    _rebind(emod, "GaussNewtonCG", _eco.gauss_newton_cg(ref, problem_cls, on_run))


def _install_gn_hinge():
    """`GNSteepestDescent` on an exact reference `LinearFilterHinge` with parameter_batch_dim=0, residual_batch_dim=1
    (dimpnet.py:236-242, rts_net.py:325-333) -> the fused solver (pytracking_amd.gn_hinge); the residual object stays the reference's.
    CPU tensors, grad-enabled inputs and uncovered shapes run the reference forward (or raise under strict=True).  Does not depend on
    the LWL modules importing."""
    from . import gn_hinge as _gh
    try:
        smod = importlib.import_module("ltr.models.meta.steepestdescent")
        hinge_cls = importlib.import_module("ltr.models.target_classifier.residual_modules").LinearFilterHinge
    except Exception:
        return
    ref_gn = smod.GNSteepestDescent

    def covered(self, meta_parameter, num_iter=None, *args, **kwargs):
        n_it = self.num_iter if num_iter is None else num_iter
        return (not args and set(kwargs) <= {"feat", "bb", "train_label", "sample_weight", "is_distractor"}
                and kwargs.get("is_distractor") is None
                and _gh.covered(self.residual_module, meta_parameter, dict(kwargs, _num_iter=n_it),
                                self._parameter_batch_dim, self._residual_batch_dim))

    class _FusedHinge(_gh.GNSteepestDescent):
        _compute_loss = ref_gn._compute_loss
        _sqr_norm = ref_gn._sqr_norm
        forward = _dispatcher(ref_gn.forward, "GNSteepestDescent.hinge", covered, _gh.GNSteepestDescent.forward,
                              "GNSteepestDescent (hinge residual): call outside the gfx950 hot path")

    _rebind(smod, "GNSteepestDescent", _choosing_class(
        ref_gn, lambda residual_module=None, *args, **kw: (type(residual_module) is hinge_cls and kw.get("residual_batch_dim", 0) == 1
                                                            and kw.get("parameter_batch_dim", 0) == 0),
        _FusedHinge, doc="LinearFilterHinge -> fused hinge solver; any other residual module -> the reference class."))


def _install_lwl():
    """LWL few-shot learner: the residual module is replaced outright (same parameters); the generic optimiser class dispatches on it.
    The hinge residual (dimp_simple, RTS classifier) is recognised by `_install_gn_hinge`'s class, which this one chains to, and kept as
    the reference's object; the RTS segmentation residual (RTSResidual, the same forward as LWTLResidual) is replaced by the LWTL mirror
    like LWTLResidual.  Any other residual module keeps the reference implementation."""
    try:
        smod = importlib.import_module("ltr.models.meta.steepestdescent")
        rmod = importlib.import_module("ltr.models.lwl.loss_residual_modules")
    except Exception:
        return
    ref_gn, ref_res = smod.GNSteepestDescent, rmod.LWTLResidual
    hinge_new = ref_gn.__new__

    class _ResMirror(_sd.LWTLResidual):
        # the residual vectors themselves (only the reference's generic forward asks for them): the reference's
        # own method on the rebound filter layer, so CPU tensors and autograd behave as upstream
        forward = ref_res.forward

    def covered(self, meta_parameter, num_iter=None, *args, **kwargs):
        w = meta_parameter[0] if isinstance(meta_parameter, (list, tuple)) else meta_parameter
        feat = kwargs.get("feat")
        return (isinstance(feat, torch.Tensor) and feat.is_cuda and w.is_cuda and not args
                and not (torch.is_grad_enabled() and (w.requires_grad or feat.requires_grad)))

    class _FusedGN(_sd.GNSteepestDescent):
        _compute_loss = ref_gn._compute_loss
        _sqr_norm = ref_gn._sqr_norm
        forward = _dispatcher(ref_gn.forward, "GNSteepestDescent", covered, _sd.GNSteepestDescent.forward,
                              "GNSteepestDescent: call outside the gfx950 hot path")

    class GNSteepestDescent(ref_gn):
        """LWTLResidual (gfx950 mirror) at inference -> fused solver; any other residual module, a training call
        (grad-enabled inputs) or CPU tensors -> the reference class / the reference forward."""

        def __new__(cls, residual_module=None, *args, **kw):
            if (isinstance(residual_module, _sd.LWTLResidual) and residual_module.filter_dilation_factors is None
                    and kw.get("residual_batch_dim", 0) == 1 and kw.get("parameter_batch_dim", 0) == 0):
                return _FusedGN(residual_module, *args, **kw)
            return hinge_new(cls, residual_module, *args, **kw)

    def undilated(init_filter_reg=1e-2, filter_dilation_factors=None):
        return filter_dilation_factors is None

    _rebind(rmod, "LWTLResidual", _choosing_class(
        ref_res, undilated, _ResMirror, "LWTLResidual: dilated filters are outside the gfx950 hot path",
        doc="No dilation factors -> the gfx950 mirror (same parameter); dilated filters -> the reference class."))
    _rebind(smod, "GNSteepestDescent", GNSteepestDescent)
    # `ltr.models.rts.loss_residual_modules.RTSResidual` (forward identical to LWTLResidual's): undilated -> the LWTL mirror, so that the
    # LWL fused solver (which reads filter_reg through the mirror's scalar cache) takes the RTS segmentation learner
    try:
        rts = importlib.import_module("ltr.models.rts.loss_residual_modules")
    except Exception:
        return
    if hasattr(rts, "RTSResidual"):
        _rebind(rts, "RTSResidual", _choosing_class(
            rts.RTSResidual, undilated, _ResMirror, "RTSResidual: dilated filters are outside the gfx950 hot path",
            doc="No dilation factors -> the gfx950 LWTL mirror (same parameter); dilated filters -> the reference class."))


def _install_atom_cg():
    """ATOM's optimisers (`pytracking.libs.optimization`) and its per-frame classification call (`_install_operation`).  `atom.atom`
    imports the two classes by name, so its names are re-pointed too."""
    try:
        pmod = importlib.import_module("pytracking.libs.optimization")
        amod = importlib.import_module("pytracking.tracker.atom.optim")
    except Exception:          # pytracking side not importable (missing cv2 ...): the ltr side is still installed
        return
    ak = _optimization.activation_kind

    def covered_cg(problem, variable, *args, **kw):
        kind = ak(getattr(problem, "response_activation", None))[0]
        return _hit("ConjugateGradient", (
            isinstance(problem, amod.ConvProblem) and kind == "mlu" and len(variable) == 1
            and variable[0].is_cuda and variable[0].shape[-1] == variable[0].shape[-2]
            and variable[0].shape[-1] ** 2 <= 16 and not kw.get("debug", False)
            and kw.get("standard_alpha", True) and kw.get("cg_eps", 0.0) == 0.0))

    def covered_gn(problem, variable, *args, **kw):
        return _hit("GaussNewtonCG", (
            isinstance(problem, amod.FactorizedConvProblem) and len(variable) == 2 and variable[0].is_cuda
            and ak(getattr(problem, "response_activation", None))[0] == "mlu"
            and ak(getattr(problem, "projection_activation", None))[0] == "identity"
            and variable[0].shape[-1] == variable[0].shape[-2] and variable[0].shape[-1] ** 2 <= 16
            and not any(kw.get(k, False) for k in ("debug", "analyze", "plotting"))
            and kw.get("standard_alpha", True) and kw.get("cg_eps", 0.0) == 0.0
            and kw.get("direction_forget_factor", 0) == 0))

    classes = (
        ("ConjugateGradient", _choosing_class(
            pmod.ConjugateGradient, covered_cg, _optimization.ConjugateGradient, "ConjugateGradient: problem outside the gfx950 hot path",
            doc="ConvProblem + MLU on device -> fused gfx950 CG; any other problem -> the reference class.")),
        ("GaussNewtonCG", _choosing_class(
            pmod.GaussNewtonCG, covered_gn, _optimization.GaussNewtonCG, "GaussNewtonCG: problem outside the gfx950 hot path",
            doc="FactorizedConvProblem, MLU response + identity projection activation, one feature block on device -> fused gfx950 joint "
                "Gauss-Newton; any other problem -> the reference class.")))
    for name, cls in classes:
        _rebind(pmod, name, cls)
    _install_operation()
    tmod = sys.modules.get("pytracking.tracker.atom.atom")
    for name, cls in classes:
        if tmod is not None and hasattr(tmod, name):
            _rebind(tmod, name, cls)


def install(strict=False, atom_cg=True, tomp=True, clf_head=True, localization=True, iou_refine=True, preprocessing=True,
            candidate_matching=True, kys=True, iou_feat=False, label_encoder=False, decoder=False, feature_heads=False,
            rts_fusion=False, seg_readout=False, eco=False, tamos=False, box_encoder=False, eco_init=False, iou_mod=False,
            tamos_readout=False, atom_localize=False, memory=False, backbone=False):
    """Rebind the boundary symbols.  Call after the reference is importable (`sys.path`) and before networks or
    trackers are constructed.  Idempotent.  If an installer raises, what was rebound so far is undone before the exception
    propagates (an optional reference module that does not import is not a failure: its family is skipped)."""
    if _state["installed"]:
        return
    mark = len(_state["ledger"])
    _state["strict"] = strict
    try:
        provide_prroi_module()                                # must precede `import ltr.models...`
        _install_filter_layer()
        _install_optimizer_classes()
        _install_gn_hinge()
        _install_lwl()                                        # chains to the hinge class: after _install_gn_hinge
        # in this order: iou_refine imports `atom.atom` before _install_atom_cg re-points the names it imported
        for flag, installer in ((tomp, _install_tomp),
                                (clf_head or feature_heads, functools.partial(_install_clf_head, feature_heads)),
                                (localization, _install_localization),
                                (iou_refine, _install_iou_refine), (preprocessing, _install_preprocessing),
                                (candidate_matching, _install_candidate_matching), (kys, _install_kys), (atom_cg, _install_atom_cg),
                                (iou_feat, _install_iou_feat), (label_encoder, _install_label_encoder),
                                (decoder, _install_lwl_decoder), (rts_fusion, _install_rts_fusion),
                                (seg_readout, _install_seg_readout), (eco, _install_eco), (tamos, _install_tamos),
                                (box_encoder, _install_box_encoder), (eco_init, _install_eco_init), (iou_mod, _install_iou_mod),
                                (tamos_readout, _install_tamos_readout), (atom_localize, _install_atom_localize),
                                (memory, _install_memory), (backbone, _install_backbone)):
            if flag:
                installer()
    except BaseException:
        _replay(mark)
        raise
    _state["installed"] = True


def uninstall():
    """Restore every binding the ledger holds, last first: an `install()`, and a `provide_*` call made on its own."""
    _replay()
    _state["installed"] = False
