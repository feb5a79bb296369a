"""The unmodified reference KYS tracker (pytracking/tracker/kys/kys.py) on the MI355X through pytracking_amd.install(), closed loop, with the
network of the train setting -- one 16-wide representation layer, conf_measure 'entropy', dimp_thresh 0.05 -- against its CPU run without
install() (tests/golden/tracker_kys.npz, recorded by tools/make_golden_kys.py tracker through tests/kys_tracker.py): same event sequence,
every payload within the compare_logs bounds, every frame's predict_response on its gfx950 branch and never on the reference's, and the
gfx950 branch taken for the rebound symbols a KYS frame reaches (filter apply, steepest-descent solver, classification head, PrRoIPool).

NOT rebound, the reference's own Python on the device: KYS.localize_target / compute_target_location and KYS.refine_target_box /
optimize_boxes_default are methods of a class install() does not touch (the IoU predictor under them runs on the rebound PrRoIPool)."""
import pytest

from oracle import ref_harness

import kys_tracker as KT
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def test_kys_on_device_matches_its_cpu_run():
    events, stats = KT.run_installed("cuda")
    dev = TOD.compare_logs(events, TOD._golden("tracker_kys"), atol=1e-4)
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print("install.stats", stats)
    frames = sum(e["kind"] == "frame" for e in events)
    assert frames == KT.RUN["n_frames"] and sum(e["kind"] == "optimize" for e in events) > 0 and sum(e["kind"] == "refine" for e in events) > 0
    assert stats.get("PredictorWrapper.predict_response.fast", 0) == frames and stats.get("PredictorWrapper.predict_response.reference", 0) == 0
    for name in KT.EXPECT_FAST:
        assert stats.get(name + ".fast", 0) > 0, f"gfx950 branch of `{name}` never taken: {stats}"
    fell = {k: v for k, v in stats.items() if k.endswith(".reference") and not k.startswith(("sample_patch", "max2d"))}
    assert not fell, f"calls handed back to the reference's own code on the device: {fell}"
