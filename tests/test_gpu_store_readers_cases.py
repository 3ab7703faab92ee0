"""ifx_map_bounding_boxes, ifx_instance_point_cloud and ifx_precision_recall on the hand-built labelled maps of tests/store_readers_cases.py, side by side with the
oracle on the same uploads: no table colour at all, every slot owning one surfel on both sides of 0, pole and seam normals, ties of the ground and heading votes,
point clouds cut at the scan's tile border, ground-truth ids around 0 and 255.  Integers (the 648 ground votes, counts, the three precision / recall tables, slots,
colours) are exact; ground normal, frames, boxes and records keep the tolerances of tests/test_gpu_parity.py::test_bounding_boxes_and_instance_point_clouds
(store_readers_cases.compare_boxes / compare_cloud).  What the uploaded arrays alone say is asserted of the HIP outputs directly as well.  Both handles are built
once per module: the instance table lives in the handle and survives an upload."""
import pytest

import store_readers_cases as sc

pytestmark = pytest.mark.gpu

UPLOADS = sc.all_uploads()


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


@pytest.fixture(scope="module")
def sheets(ifx, orc):
    o = sc.oracle_sheet(orc)
    g, inst = sc.hip_sheet(ifx)
    yield o, g, inst
    g.close(); o.close()


@pytest.mark.parametrize("up", UPLOADS, ids=[u["name"] for u in UPLOADS])
def test_hip_against_the_oracle(sheets, up):
    o, g, inst = sheets
    want = sc.run_oracle(o, up)
    got = sc.run_hip(g, inst, up)
    assert g.slots == g.count == up["m"]["pc"].shape[0]                     # an uploaded map: no holes (tests/test_gpu_store_readers.py has them)
    for a, b, name in zip(got["pr"], want["pr"], ("inst_num", "gt_num", "inst_gt_map")):
        assert (a == b).all(), (up["name"], name)
    assert (got["counts"] == want["counts"]).all(), up["name"]
    for key in want["boxes"]:
        sc.compare_boxes(got["boxes"][key], want["boxes"][key], (up["name"],) + key)
    for key in want["clouds"]:
        sc.compare_cloud(got["clouds"][key], want["clouds"][key], (up["name"],) + key)
    sc.compare_with_construction(got, up)
