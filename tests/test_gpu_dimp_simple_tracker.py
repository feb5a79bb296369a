"""The unmodified reference DiMPSimple tracker on the MI355X through pytracking_amd.install(), closed loop, against its CPU run without
install() (tests/golden/tracker_dimp_simple.npz, recorded by tools/make_golden_gn_hinge.py through tests/dimp_simple_tracker.py):
same event sequence, every payload within the compare_logs bounds, and every rebound symbol of a dimp_simple frame on its gfx950
branch (the reference branch never taken on the device)."""
import numpy as np
import pytest

from oracle import ref_harness

import dimp_simple_tracker as DST
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def test_dimp_simple_on_device_matches_its_cpu_run():
    events, stats = DST.run_installed("cuda")
    dev = TOD.compare_logs(events, TOD._golden("tracker_dimp_simple"), atol=1e-4)
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print("install.stats", stats)
    assert sum(e["kind"] == "optimize" for e in events) > 0 and sum(e["kind"] == "refine" for e in events) > 0
    for name in DST.EXPECT_FAST:
        assert stats.get(name + ".fast", 0) > 0, f"gfx950 branch of `{name}` never taken: {stats}"
    fell = {k: v for k, v in stats.items() if k.endswith(".reference") and not k.startswith(("sample_patch", "max2d"))}
    assert not fell, f"calls handed back to the reference's own code on the device: {fell}"
    # the tracker module's own sample_patch* names are the rebound ones (host images take their reference branch)
    assert any(k.startswith("sample_patch") for k in stats), stats
