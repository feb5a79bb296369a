"""The unmodified reference TaMOs tracker (pytracking/tracker/tamos/tamos.py) on the MI355X through
pytracking_amd.install(tamos=True, tamos_readout=True), closed loop on the stub net of tests/tamos_tracker.py -- three objects whose blobs
move, two of them cross, one vanishes for a frame -- against its CPU run without install() (tests/golden/tracker_tamos.npz, recorded by
tools/make_golden_tamos_readout.py tracker): the same event sequence; every object's flag and cell equal; boxes, the training targets handed
to the filter predictor (stored labels, encode_bbox of the stored boxes), the memory after every update and the output boxes within the
compare_logs bounds; every one of the five rebound methods on its gfx950 branch in every call and never on the reference's.

Still the reference's own per-object device reductions in track(): `scores_raw[:, :, oid-1].max() > conf_ths` (tamos.py:198) and
`score_map.max().cpu().item()` (tamos.py:216)."""
import pytest

from oracle import ref_harness

import tamos_tracker as TT
import trackers_on_device as TOD

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref_harness.available(), reason="no reference tree / bundle (oracle/_ref)")]


def test_tamos_on_device_matches_its_cpu_run():
    events, stats = TT.run_installed("cuda")
    golden = TOD._golden("tracker_tamos")
    dev = TOD.compare_logs(events, golden, atol=1e-4)
    print("max deviation per boundary payload", {k: f"{v:.2e}" for k, v in sorted(dev.items())})
    print("install.stats", stats)
    frames = sum(e["kind"] == "frame" for e in events)
    objects = [e for e in events if e["kind"] == "object"]
    assert frames == TT.RUN["n_frames"] and len(objects) == 3 * frames and sum(e["kind"] == "memory" for e in events) >= 4
    assert {str(e["flag"]) for e in objects} == {"normal", "hard_negative", "uncertain", "not_found"}       # every outcome occurs in the run
    assert stats.get("TaMOs.classify_target.fast", 0) == frames and stats.get("TaMOs.localize_target.fast", 0) == 3 * frames
    assert stats.get("TaMOs.direct_bbox_regression.fast", 0) == 3 * frames
    for name in TT.EXPECT_FAST:
        assert stats.get(name + ".fast", 0) > 0, f"gfx950 branch of `{name}` never taken: {stats}"
    fell = {k: v for k, v in stats.items() if k.endswith(".reference")}
    assert not fell, f"calls handed back to the reference's own code on the device: {fell}"
