"""The unmodified reference KeepTrack tracker on the MI355X through pytracking_amd.install(), closed loop, against its CPU run without
install() (tests/golden/tracker_keep_track.npz, recorded by tools/make_golden_keep_track.py through tests/keep_track_tracker.py): same
event sequence, every payload (candidate peaks, descriptors, matcher outputs, scores, boxes) within the compare_logs bounds, and every
rebound symbol of a keep_track frame on its gfx950 branch (the reference branch never taken on the device)."""
import pytest

from oracle import ref_harness

import keep_track_tracker as KT
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def test_keep_track_on_device_matches_its_cpu_run():
    events, stats = KT.run_installed("cuda")
    dev = TOD.compare_logs(events, TOD._golden("tracker_keep_track"), atol=1e-4)
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print("install.stats", stats)
    assert sum(e["kind"] == "match" and max(int(e["m"]), int(e["n"])) >= 2 for e in events) >= 3
    assert sum(e["kind"] == "refine" for e in events) > 0
    for name in KT.EXPECT_FAST:
        assert stats.get(name + ".fast", 0) > 0, f"gfx950 branch of `{name}` never taken: {stats}"
    fell = {k: v for k, v in stats.items() if k.endswith(".reference") and not k.startswith(("sample_patch", "max2d"))}
    assert not fell, f"calls handed back to the reference's own code on the device: {fell}"
    assert any(k.startswith("sample_patch") for k in stats), stats
