"""The unmodified reference trackers closed loop on the MI355X through pytracking_amd.install(memory=True): DiMP, ToMP, ATOM and LWL
(oracle/tracker_harness.run_*), KeepTrack (tests/keep_track_tracker.py) and TaMOs (tests/tamos_tracker.py), each with the switches it
already needs.  Every `update_memory` of the run goes through libpt_mem -- `<Class>.update_memory.fast` counts every call, `.reference` none
-- and the recorded CPU golden's event sequence is met within the compare_logs bounds: later filters depend on what was inserted where
(TaMOs's harness also records the slot, the stored label and box and the sample weights of every update).  ToMP's harness memory holds 2
samples and TaMOs's 4, so the full-memory arg-min and its one wait run there; DiMP, ATOM, LWL and KeepTrack stay in the fill phase, where
no update waits.  KYS, DiMPSimple and RTS have no closed-loop harness: their drop-ins are held by the bare-object method goldens
(tests/test_gpu_mem_update.py, tests/test_mem_update_cpu.py)."""
import numpy as np
import pytest

from oracle import ref_harness

import tracker_replay as TR
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def _counted(cls):
    """count the calls of the class's (rebound) `update_memory`"""
    calls, bound = [], vars(cls)["update_memory"]

    def update_memory(self, *args, **kw):
        calls.append(1)
        return bound(self, *args, **kw)
    cls.update_memory = update_memory
    return calls, lambda: setattr(cls, "update_memory", bound)


def _run(which):
    from oracle import tracker_harness as TH
    TH.ref_harness.install()
    from pytracking_amd import install as amd
    from pytracking_amd import memory_update as MU
    import importlib
    name = {"dimp": "DiMP", "tomp": "ToMP", "atom": "ATOM", "lwl": "LWL", "keep_track": "KeepTrack", "tamos": "TaMOs"}[which]
    cls = getattr(importlib.import_module(MU.TABLE[name].module), name)
    amd.uninstall()
    amd.install(memory=True, **({"tamos": True, "tamos_readout": True} if which == "tamos" else {}))
    amd.stats.clear()
    calls, undo = _counted(cls)
    ctx = MU.context("cuda:0")
    waits = ctx.waits
    try:
        if which == "keep_track":
            import keep_track_tracker as KT
            _, rec, _ = KT.run(device="cuda", **KT.RUN)
        elif which == "tamos":
            import tamos_tracker as TT
            rec, _ = TT.run(device="cuda", **TT.RUN)
        else:
            runner, kw = {"dimp": (TH.run_dimp, TH.DIMP_RUN), "tomp": (TH.run_tomp, TH.TOMP_RUN), "atom": (TH.run_atom, TH.ATOM_RUN),
                          "lwl": (TH.run_lwl, TH.LWL_RUN)}[which]
            _, rec, _ = runner(device="cuda", **kw)
        stats = dict(amd.stats)
    finally:
        undo()
        amd.uninstall()
    events = TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    return name, events, stats, len(calls), ctx.waits - waits


GOLDEN = dict(TOD.GOLDEN_NAME, keep_track="tracker_keep_track", tamos="tracker_tamos")


@pytest.mark.parametrize("which", ["dimp", "tomp", "atom", "lwl", "keep_track", "tamos"])
def test_tracker_runs_closed_loop_with_the_memory_update_on_the_device(which):
    name, events, stats, calls, waits = _run(which)
    golden = TOD._golden(GOLDEN[which])
    dev = TOD.compare_logs(events, golden, atol=1e-4, overrides=TOD.STOCK_OVERRIDES.get(which))
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print(f"{name}: {calls} update frames, {waits} waited; install.stats", {k: v for k, v in stats.items() if "update_memory" in k})
    assert calls > 0 and stats.get(name + ".update_memory.fast", 0) == calls and name + ".update_memory.reference" not in stats
    if which == "tamos":
        assert calls == sum(e["kind"] == "memory" for e in golden)
    if which in ("tomp", "tamos"):
        assert waits > 0                                                       # the memory fills up during the run: the arg-min ran on the device
    assert waits <= calls
