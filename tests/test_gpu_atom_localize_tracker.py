"""The unmodified reference ATOM tracker (pytracking/tracker/atom/atom.py) closed loop on the MI355X through
pytracking_amd.install(atom_localize=True), with torch.rfft / torch.irfft ABSENT: the stand-in oracle/ref_harness.py installs for the
reference's Fourier calls is taken away once the harness is set up (as tests/test_eco_cpu.py does), so every frame's localisation has to
come from libpt_loc -- the reference method would raise AttributeError.  Against the CPU run without install() (tests/golden/tracker_atom18.npz):
the same event sequence; flag and scale_ind of every frame equal, translation vectors and every other boundary payload within the
compare_logs bounds (flat 1e-4 plus the relative coordinate term); `ATOM.localize_target` on its gfx950 branch in every frame and never
handed to the reference.

Still the reference's Python in track(): `torch.max(score_map).item()` (atom.py:257), `update_state`, the memory update."""
import numpy as np
import pytest
import torch

from oracle import ref_harness

import tracker_replay as TR
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def test_atom_runs_closed_loop_without_torch_rfft(monkeypatch):
    from oracle import tracker_harness as TH
    TH.ref_harness.install()
    from pytracking_amd import install as amd
    monkeypatch.delattr(torch, "rfft", raising=False)
    monkeypatch.delattr(torch, "irfft", raising=False)
    assert not hasattr(torch, "rfft") and not hasattr(torch, "irfft")
    amd.uninstall()
    amd.install(atom_localize=True)
    amd.stats.clear()
    try:
        outs, rec, _ = TH.run_atom(device="cuda", **TH.ATOM_RUN)
        stats = dict(amd.stats)
    finally:
        amd.uninstall()
    events = TR.events_from_npz({k: np.asarray(v) for k, v in rec.to_npz_dict().items()})
    golden = TOD._golden("tracker_atom18")
    dev = TOD.compare_logs(events, golden, atol=1e-4)
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print("install.stats", stats)
    frames = TH.ATOM_RUN["n_frames"]
    got = [e for e in events if e["kind"] == "atom_localize"]
    want = [e for e in golden if e["kind"] == "atom_localize"]
    assert len(got) == len(want) == frames and outs.shape == (frames, 4) and np.isfinite(outs).all()
    for a, b in zip(got, want):
        assert str(a["flag"]) == str(b["flag"]) and int(a["scale_ind"]) == int(b["scale_ind"])
        assert np.abs(np.asarray(a["tv"], np.float64) - np.asarray(b["tv"], np.float64)).max() <= 1e-4
    assert stats.get("ATOM.localize_target.fast", 0) == frames and "ATOM.localize_target.reference" not in stats
    for name in TOD.EXPECT_FAST["atom"]:
        assert stats.get(name + ".fast", 0) > 0, f"gfx950 branch of `{name}` never taken: {stats}"
