"""install() / uninstall() as a whole against the real reference tree (CPU): the rebinding ledger restores every binding, a failed
install() rolls back, the set of rebound symbols is pinned, and `strict=True` raises where the module docstring says it does.
Runs only where the reference tree is present, like tests/test_install_reference.py."""
import json
import os
import sys

import pytest
import torch

from oracle import ref_harness

pytestmark = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not mounted")

_ROOTS = ("ltr", "pytracking", "pytracking_amd", "spatial_correlation_sampler")
_PRROI = "ltr.external.PreciseRoIPooling.pytorch.prroi_pool"
OPTIONAL = ("atom_cg", "tomp", "clf_head", "localization", "iou_refine", "preprocessing", "candidate_matching", "kys")
REBOUND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "install_rebound_symbols.json")


def snapshot():
    """{dotted name: object} of every `sys.modules` entry of the reference's and our packages, every attribute of those modules and every
    class attribute of the classes defined in them.  Values are the objects themselves: they are compared by identity."""
    snap = {}
    for modname, mod in list(sys.modules.items()):
        if modname.split(".")[0] not in _ROOTS or mod is None:
            continue
        snap[f"sys.modules[{modname}]"] = mod
        for attr, val in list(vars(mod).items()):
            snap[f"{modname}.{attr}"] = val
            if isinstance(val, type) and val.__module__ == modname:
                for k, v in list(vars(val).items()):
                    snap[f"{modname}.{attr}.{k}"] = v
    return snap


def changed(before, after):
    """Sorted names that are new, missing or bound to another object.  A name below one that is listed itself (the attributes of a
    replaced class or of a module that came or went) is left out: it says nothing more."""
    raw = {k for k in before.keys() | after.keys() if k not in before or k not in after or before[k] is not after[k]}

    def below_listed(name):
        parts = name.split(".")
        owners = [".".join(parts[:i]) for i in range(1, len(parts))]
        return not name.startswith("sys.modules[") and any(o in raw or f"sys.modules[{o}]" in raw for o in owners)
    return sorted(k for k in raw if not below_listed(k))


@pytest.fixture()
def amd():
    """The install module after one warm-up round trip (every module install() imports is in `sys.modules`); uninstalled afterwards."""
    ref_harness.install()
    from pytracking_amd import install as amd
    amd.install()
    amd.uninstall()
    try:
        yield amd
    finally:
        amd.uninstall()


@pytest.mark.parametrize("kw", [{}, {"strict": True}] + [{flag: False} for flag in OPTIONAL], ids=lambda kw: "-".join(kw) or "defaults")
def test_round_trip_restores_every_binding(amd, kw):
    before = snapshot()
    amd.install(**kw)
    assert amd.installed()
    amd.uninstall()
    assert not amd.installed()
    assert changed(before, snapshot()) == []


def test_created_prroi_module_and_parent_attribute_are_removed(amd):
    parent = sys.modules["ltr.external.PreciseRoIPooling.pytorch"]
    saved_mod, saved_attr = sys.modules.pop(_PRROI, None), parent.__dict__.pop("prroi_pool", None)
    try:
        amd.install()
        assert sys.modules[_PRROI] is parent.prroi_pool
        amd.uninstall()
        assert _PRROI not in sys.modules and "prroi_pool" not in vars(parent)
    finally:
        amd.uninstall()
        if saved_mod is not None:
            sys.modules[_PRROI] = saved_mod
        if saved_attr is not None:
            parent.prroi_pool = saved_attr


def test_rebound_set_is_pinned(amd):
    """install() with default arguments rebinds exactly the names recorded before the ledger was introduced."""
    before = snapshot()
    amd.install()
    got = changed(before, snapshot())
    with open(REBOUND) as fh:
        assert got == json.load(fh)


def test_failed_install_rolls_back(amd, monkeypatch):
    before = snapshot()

    def boom(*args, **kw):
        raise RuntimeError("installer failed")
    with monkeypatch.context() as m:
        m.setattr(amd, "_install_kys", boom)
        with pytest.raises(RuntimeError, match="installer failed"):
            amd.install()
    assert not amd.installed()
    assert changed(before, snapshot()) == []
    amd.install()
    assert amd.installed()
    amd.uninstall()
    assert changed(before, snapshot()) == []


def test_strict_mode_on_cpu_tensors(amd):
    import ltr.models.layers.filter as fl
    import ltr.data.processing_utils as prutils
    import ltr.models.lwl.loss_residual_modules as rmod
    import ltr.models.transformer.transformer as rt
    import pytracking.features.preprocessing as pp
    import pytracking.libs.dcf as dcf
    import pytracking.libs.operation as op
    feat, filt = torch.randn(2, 1, 8, 6, 6), torch.randn(1, 8, 4, 4)
    scores = torch.randn(2, 1, 7, 7)
    im, pos, sz = torch.rand(1, 3, 24, 32) * 255, torch.Tensor([12.0, 16.0]), torch.Tensor([16.0, 16.0])
    x, w = torch.randn(3, 8, 9, 9), torch.randn(1, 8, 4, 4)
    want_patch, want_conv = pp.sample_patch(im, pos, sz), op.conv2d(x, w, mode='same')
    amd.install(strict=True)
    P = "configuration outside the gfx950 hot path"
    for name, call, message in (
            ("apply_filter", lambda: fl.apply_filter(feat, filt), "apply_filter: " + P),
            ("apply_feat_transpose", lambda: fl.apply_feat_transpose(feat, scores, 4, training=False), "apply_feat_transpose: " + P),
            ("filter_gradient", lambda: fl.filter_gradient(feat, filt), "filter_gradient: " + P),
            ("max2d", lambda: dcf.max2d(torch.randn(2, 7, 9)), "max2d: tensor outside the gfx950 hot path"),
            ("find_local_maxima", lambda: prutils.find_local_maxima(torch.randn(1, 1, 9, 9), th=0.1, ks=3),
             "find_local_maxima: call outside the gfx950 hot path")):
        amd.stats.clear()
        with pytest.raises(NotImplementedError) as exc:
            call()
        assert str(exc.value) == message
        assert dict(amd.stats) == {name + ".reference": 1}
    # the rebound classes that choose an implementation when they are constructed: no per-call counter, the refusal is the check
    with pytest.raises(NotImplementedError) as exc:
        rmod.LWTLResidual(filter_dilation_factors=[1, 2])
    assert str(exc.value) == "LWTLResidual: dilated filters are outside the gfx950 hot path"
    with pytest.raises(NotImplementedError) as exc:
        rt.Transformer(normalize_before=True, d_model=128, nhead=4, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=256)
    assert str(exc.value) == "Transformer: " + P
    # strict refuses device calls only for the patch samplers and operation.conv2d: CPU images / tensors keep the reference's result
    got, _ = pp.sample_patch(im, pos, sz)
    assert torch.equal(got, want_patch[0])
    assert torch.equal(op.conv2d(x, w, mode='same'), want_conv)


def test_install_and_uninstall_are_idempotent(amd):
    import pytracking.libs.optimization as po
    ref_cg = po.ConjugateGradient
    before = snapshot()
    amd.install()
    once, entries = snapshot(), len(amd._state["ledger"])
    amd.install()
    assert len(amd._state["ledger"]) == entries and changed(once, snapshot()) == []
    assert amd.original(po, "ConjugateGradient") is ref_cg
    amd.uninstall()
    after = snapshot()
    amd.uninstall()
    assert changed(before, after) == [] and changed(after, snapshot()) == []
