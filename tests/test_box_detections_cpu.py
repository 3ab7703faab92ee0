"""The numpy statement of the box head's post-processing (tests/box_detections_numpy.py) against maskrcnn-benchmark's own Python
(tests/golden/box_detections_ref.npz, written by tools/make_golden_box_detections.py), its softmax against the f64 value and at the rows that yield nothing, the
limit with ties, and what needs no GPU of the interfaces: the binding's argument checks, the symbol in header, library and binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import box_detections_cases as bc
import box_detections_numpy as bd
import rpn_proposals_numpy as rp
from conftest import ROOT

F = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_detections_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_the_statement_has_the_references_detections(golden):
    """Equal count, equal labels and proposal rows in equal order; every coordinate within 2 ulp of the largest magnitude among pcx, pcy, pw and ph of its box (the
    RPN tool's unit and bound); every probability of the statement within 3 ulp of exp(d_j) / sum exp(d_i) in f64 -- one rounding each from EXP, the sum and the
    conversion.  The largest distances seen are the golden file's."""
    worst_box, worst = 0.0, np.zeros(3)
    detections, above, below = 0, 0, 0
    shapes, agnostic = set(), 0
    for k in range(int(golden["counts"][0])):
        logits, reg, prop, weights = golden[f"det{k}_logits"], golden[f"det{k}_regression"], golden[f"det{k}_proposals"], tuple(golden[f"det{k}_weights"])
        iw, ih, st, nms, M, K, Dk = golden[f"det{k}_par"]
        boxes, scores, labels, index, K2, D2 = bd.box_detections(logits, reg, prop, (int(iw), int(ih)), st, nms, int(M), weights)
        ref = golden[f"det{k}_boxes"]
        assert (K2, D2) == (int(K), int(Dk)) and K2 <= bd.CAP
        assert boxes.shape == ref.shape and np.array_equal(labels, golden[f"det{k}_labels"]) and np.array_equal(index, golden[f"det{k}_index"]), k
        creg = reg.shape[1] // 4
        agnostic += creg == 1 and logits.shape[1] > 1
        if index.size:
            codes = reg.reshape(-1, creg, 4)[index, labels if creg > 1 else 0]
            unit = rp.coordinate_ulp(codes, prop[index], weights)
            err = float((np.abs(boxes.astype(np.float64) - ref) / unit).max())
            assert err <= 2.0, (k, err)
            worst_box = max(worst_box, err)
        p, true = bd.softmax(logits), bd.softmax_true(logits)
        d_stmt = float(bd.ulp_distance(p, true).max())
        assert d_stmt <= 3.0, (k, d_stmt)
        worst[0] = max(worst[0], d_stmt)
        if index.size:                                                                 # the reference's scores: torch's softmax, measured, not bounded here
            worst[1] = max(worst[1], float(bd.ulp_distance(golden[f"det{k}_scores"], true[index, labels]).max()))
            unit = np.spacing(np.abs(true[index, labels]).astype(F)).astype(np.float64)
            worst[2] = max(worst[2], float((np.abs(scores.astype(np.float64) - golden[f"det{k}_scores"]) / unit).max()))
        detections += index.size
        above += int(M > 0 and D2 > M)
        below += int(M > 0 and D2 < M)
        shapes.add(logits.shape[1])
    stored = golden["worst_softmax_ulp"]
    print(f"{detections} detections; coordinates within {worst_box:.3f} of the unit (the tool saw {golden['worst_box_ulp'][0]:.3f}; bound 2); softmax: statement "
          f"{worst[0]:.3f} ulp (the tool saw {stored[0]:.3f}; bound 3); the kept scores: torch {worst[1]:.3f} ulp, statement to torch {worst[2]:.3f} ulp "
          f"(over every probability the tool saw {stored[1]:.3f} and {stored[2]:.3f})")
    assert shapes == {2, 3, 81} and agnostic == 1 and detections > 500 and above >= 3 and below >= 3
    assert detections == int(golden["counts"][2]) and (above, below) == (int(golden["counts"][3]), int(golden["counts"][4]))
    assert worst_box == golden["worst_box_ulp"][0] and worst[0] == stored[0]
    assert worst[1] <= stored[1] and worst[2] <= stored[2] <= stored[0] + stored[1]


def test_softmax_is_within_three_ulp_of_the_f64_value():
    rng = np.random.default_rng(5)
    worst = 0.0
    for C_ in (2, 3, 17, 81, 333, 1000):
        x = (rng.standard_normal((60, C_)) * rng.uniform(0.2, 8, (60, 1))).astype(F)
        p = bd.softmax(x)
        assert p.dtype == F and (p[np.arange(60), x.argmax(axis=1)] > 0).all()
        worst = max(worst, float(bd.ulp_distance(p, bd.softmax_true(x)).max()))
    print(f"largest distance {worst:.3f} ulp (bound 3)")
    assert worst <= 3.0
    d, e, bad = bd.softmax_parts(np.asarray([[1.0, 3.0, 3.0, -np.inf]], F))
    assert not bad[0] and e[0, 1] == 1 and e[0, 2] == 1 and e[0, 3] == 0              # e at the maximum is exactly 1; EXP's clamp at -104 rounds to 0
    assert np.array_equal(bd.softmax(np.asarray([[0.0, 0.0]], F)), np.asarray([[0.5, 0.5]], F))


def test_rows_that_yield_no_candidate():
    """a NaN in the row, a +inf logit and an all -inf row: every probability is a NaN (torch's whole-row NaN) and no candidate comes from the row"""
    logits, reg, prop, img = bc.head(7, 6, 5, scale=1.0)
    clean = bd.box_detections(logits, reg, prop, img, 0.05, 2.0, 0)
    assert {0, 1, 2, 3, 4, 5} == set(clean[3].tolist())
    logits[1, 2] = np.nan
    logits[3, 4] = np.inf
    logits[4, :] = -np.inf
    logits[5, 0] = -np.inf                                                            # a -inf beside numbers is an ordinary 0
    p = bd.softmax(logits)
    assert np.isnan(p[[1, 3, 4]]).all() and not np.isnan(p[[0, 2, 5]]).any() and p[5, 0] == 0
    import torch

    tp = torch.nn.functional.softmax(torch.from_numpy(logits), -1).numpy()
    assert np.array_equal(np.isnan(tp), np.isnan(p))
    got = bd.box_detections(logits, reg, prop, img, 0.05, 2.0, 0)
    assert set(got[3].tolist()) == {0, 2, 5}
    keep = np.isin(clean[3], [0, 2])
    rows02 = np.isin(got[3], [0, 2])
    assert np.array_equal(got[0][rows02], clean[0][keep]) and np.array_equal(got[1][rows02], clean[1][keep])
    none = bd.box_detections(np.full((4, 3), np.nan, F), reg[:4, :12], prop[:4], img)
    assert none[0].shape == (0, 4) and none[4:] == (0, 0)
    pb, ps, pl, pi, c, stats = bd.padded(none, 7)
    assert c == 0 and not pb.any() and not ps.any() and (pl == -1).all() and (pi == -1).all() and stats.tolist() == [0, 0]


def test_candidate_order_is_class_major_and_the_kept_stay_in_it():
    logits, reg, prop, img = bc.head(8, 40, 4, scale=1.0)
    boxes, scores, labels, index = bd.candidates(logits, reg, prop, img, 0.05)
    assert (np.diff(labels) >= 0).all() and all((np.diff(index[labels == j]) > 0).all() for j in (1, 2, 3))
    p = bd.softmax(logits)
    assert scores.size == int((p[:, 1:] > F(0.05)).sum()) and np.array_equal(scores, p[index, labels])
    full = rp.box_decode(reg, prop, bc.WEIGHTS, clip_to=img).reshape(40, 4, 4)
    assert np.array_equal(boxes, full[index, labels])
    b, s, l, i, K, Dk = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 0)
    assert 0 < Dk < K and (np.diff(l) >= 0).all() and all((np.diff(i[l == j]) > 0).all() for j in (1, 2, 3))
    per_class = [bd.nms(boxes[labels == j], scores[labels == j], 0.5) for j in (1, 2, 3)]       # the reference's loop over the classes
    assert np.array_equal(i, np.concatenate([index[labels == j][kp] for j, kp in zip((1, 2, 3), per_class)]))


def test_cls_agnostic_uses_the_one_code_for_every_class():
    logits, reg, prop, img = bc.head(9, 30, 5, creg=1)
    assert reg.shape == (30, 4)
    a = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 10)
    b = bd.box_detections(logits, np.tile(reg, (1, 5)), prop, img, 0.05, 0.5, 10)
    assert a[0].shape[0] >= 10 and all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4:] == b[4:]


def test_the_limit_keeps_every_tie_at_the_threshold():
    """quantised logits: many kept scores tie at t, all of them stay and the count exceeds M; the padded form writes max_out rows"""
    rng = np.random.default_rng(10)
    R = 60
    logits = np.zeros((R, 3), F)
    logits[:, 1] = rng.integers(0, 3, R).astype(F)                                    # three distinct probabilities of class 1
    reg, prop = np.zeros((R, 12), F), (np.arange(R, dtype=F)[:, None] * 40 + np.asarray([0, 0, 20, 20], F)).astype(F)      # far apart: nothing is suppressed
    img = (4000, 100)
    free = bd.box_detections(logits, reg, prop, img, 0.3, 0.5, 0)
    assert free[5] == free[0].shape[0] == free[4] > 30
    vals = np.unique(free[1])[::-1]
    top = int((free[1] == vals[0]).sum())
    assert vals.size >= 2 and 2 <= top
    M = top + 1                                                                        # the M-th largest is the second value: all of its ties stay
    got = bd.box_detections(logits, reg, prop, img, 0.3, 0.5, M)
    t = bd.limit_threshold(free[1], M)
    assert t == vals[1] and got[0].shape[0] == int((free[1] >= vals[1]).sum()) > M and got[5] == free[5]
    assert np.array_equal(got[3], free[3][free[1] >= t]) and (np.diff(got[3][got[2] == 1]) > 0).all()
    pb, ps, pl, pi, c, stats = bd.padded(got, M)
    assert c == got[0].shape[0] > M and np.array_equal(pi, got[3][:M]) and (pl >= 1).all()
    exact = bd.box_detections(logits, reg, prop, img, 0.3, 0.5, top)                   # t = the first value: exactly its ties
    assert exact[0].shape[0] == top
    assert bd.box_detections(logits, reg, prop, img, 0.3, 0.5, free[5])[0].shape[0] == free[5]      # D == M: no cut
    assert bd.box_detections(logits, reg, prop, img, 0.3, 0.5, free[5] + 1)[0].shape[0] == free[5]  # D < M
    one = bd.box_detections(logits, reg, prop, img, 0.3, 0.5, 1)
    assert one[0].shape[0] == top                                                      # M = 1: the maximum and its ties


def test_above_the_cap():
    logits, reg, prop, img = bc.at_the_cap(4097)
    got = bd.box_detections(logits, reg, prop, img, 0.05, 0.5, 100)
    assert got[4:] == (8194, 0) and got[0].shape == (0, 4)
    pb, ps, pl, pi, c, stats = bd.padded(got, 100)
    assert c == -1 and stats.tolist() == [8194, 0] and not pb.any() and (pi == -1).all()
    assert bd.candidates(*bc.at_the_cap(4096), 0.05)[1].size == 8192
    for K in (0, 1, 63, 64, 65):
        assert bd.candidates(*bc.with_k(K, 64 if K else 5, 3, K), 0.05)[1].size == K


def _bare(ifx):
    """an ElasticFusion object without a handle: the argument checks in front of the C call need none"""
    ef = object.__new__(ifx.ElasticFusion)
    ef.cfgd = {"device": 0}
    ef.handle = None
    return ef


def test_the_bindings_argument_checks_need_no_gpu():
    import torch

    import instancefusion_amd as ifx

    ef = _bare(ifx)
    lg, rg, pr = torch.zeros(5, 3), torch.zeros(5, 12), torch.zeros(5, 4)
    with pytest.raises(TypeError, match="torch tensor"):
        ef.box_detections(lg.numpy(), rg, pr, (10, 10))
    with pytest.raises(TypeError, match="float16"):
        ef.box_detections(lg.half(), rg, pr, (10, 10))
    with pytest.raises(TypeError, match="float64"):
        ef.box_detections(lg.double(), rg, pr, (10, 10))
    with pytest.raises(ValueError, match="is on cpu"):
        ef.box_detections(lg, rg, pr, (10, 10))
    pp = ifx.box_post_processor(ef, 0.05, 0.5, 100, cls_agnostic_bbox_reg=True)
    assert pp.weights == (10.0, 10.0, 5.0, 5.0) and pp.cls_agnostic_bbox_reg and isinstance(pp, torch.nn.Module)
    with pytest.raises(RuntimeError, match="inference only"):
        pp.train()((lg, rg), [])
    assert pp.eval()((lg, rg), []) == []


def test_symbol_in_header_library_binding_and_host_class():
    import instancefusion_amd as ifx

    header = open(ifx.HEADER_PATH).read()
    assert re.search(r"\bint ifx_box_detections\(ifx_t\* h, const float\* d_logits", header) and "} ifx_box_det_params;" in header
    assert "ifx_box_detections" in ifx.exported_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", ifx.LIB_PATH]).decode()
    assert re.search(r"\bT ifx_box_detections\b", out)
    assert C.sizeof(ifx.BoxDetParams) == 44 and [f[0] for f in ifx.BoxDetParams._fields_] == ["score_thresh", "nms", "detections_per_img", "max_out", "weights",
                                                                                               "xform_clip", "image_w", "image_h"]
    fields = re.search(r"typedef struct ifx_box_det_params \{(.*?)\} ifx_box_det_params;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields)
    assert re.findall(r"(\w+)(?:\[4\])?\s*[,;]", fields) == [f[0] for f in ifx.BoxDetParams._fields_]
    host = open(os.path.join(ROOT, "instancefusion_amd", "host", "ifx_host.hpp")).read()
    assert "void BoxDetections(" in host and "ifx_box_detections(h_" in host
    assert ifx.lib().ifx_box_detections.argtypes[7]._type_ is ifx.BoxDetParams
