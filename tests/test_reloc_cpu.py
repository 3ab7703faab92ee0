"""The relocalisation scenario on the reference driver alone (tests/reloc_reference.py, CPU oracle): the inputs of tests/test_gpu_reloc.py are adequate --
tracking really fails on the masked frames, the map is really lost and really recovers -- and the driver's composition of the oracle's stage calls reproduces
orc_process_frame where no option is set."""
import numpy as np

import reloc_reference as rr


def test_driver_reproduces_process_frame(orc):
    """No option set: tracker + process_frame(in_pose = tracked pose) gives orc_process_frame's poses and map bit for bit."""
    st = rr.scenario_stream()
    d = rr.RelocReference(orc, reloc=False, loop_closure=False, **rr.SCENARIO)
    o = orc.Oracle(max_surfels=1 << 18, **rr.SCENARIO)
    for i in range(5):
        r = d.frame(st["rgb"][i], st["depth"][i])
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        assert np.array_equal(r["pose"], po), f"frame {i}"
    assert d.o.count == o.count
    ma, mb = d.o.download(), o.download()
    for k in ma:
        assert np.array_equal(ma[k], mb[k]), k


def test_scenario_is_adequate(orc):
    st, recs, maps, ids, d = rr.scenario_run(orc)
    for i, r in enumerate(recs):
        print(f"frame {i:2d}: err {r['err']:.3e} cov {np.max(r['cov_diag']):.3e} ok {int(r['ok'])} lost {int(r['lost'])} rec {int(r['recovery'])} count {r['count']:2d} "
              f"tick {r['tick']:2d} surfels {r['surfels']} fused {int(r['fused'])}")
        assert np.isfinite(r["pose"]).all(), f"NaN pose at frame {i}"
    # both gates are clearly on one side on every frame (at least 10 % away from the thresholds -- the errors are sums that agree to f32 rounding on both sides: no verdict hangs on a rounding)
    for i, r in enumerate(recs[1:], 1):
        cm = float(np.max(r["cov_diag"]))
        if 6 <= i <= 18:
            assert not r["ok"] and r["err"] > 1.1e-4 and cm > 1.1e-4, (i, r["err"], cm)
        else:
            assert r["err"] < 0.9e-4 and cm < 0.9e-4, (i, r["err"], cm)
    assert [i for i, r in enumerate(recs) if r["lost"]] == [16, 17, 18, 19], "lost at frame 16 (count 11) and not before; cleared by frame 20"
    assert recs[16]["count"] == 11 and recs[15]["count"] == 10 and not recs[15]["lost"]
    assert [r["tick"] for r in recs[15:21]] == [17, 17, 17, 17, 17, 18], "the tick stands still while lost"
    assert recs[19]["recovery"] and not recs[18]["recovery"] and not recs[20]["recovery"]
    assert all(not r["fused"] for r in recs[6:20]) and all(r["fused"] for r in recs[:6] + recs[20:])
    assert len({r["surfels"] for r in recs[5:20]}) == 1, "the map does not change while frames are skipped"
    assert recs[20]["ok"] and not recs[20]["lost"] and recs[20]["surfels"] > recs[19]["surfels"], "frame 20 clears lost and fuses again"
    assert np.array_equal(recs[19]["pose"], np.asarray(st["poses"][19], np.float32)), "frame 19 adopted the recovery pose"
