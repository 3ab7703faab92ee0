"""The numpy statement of the device entry's ingestion (tests/mask_bridge_numpy.py) without a GPU: against the literal bridge expression of
tests/test_gpu_seg_device_masks.py (build/mask_ori.py:87-124), its overlap clean against the oracle's orc_mask_clean_overlap, the inside rule at its edges, and
the stage entry ifx_ingest_masks in the header and the binding."""
import ctypes as C
import re

import numpy as np

import mask_bridge_numpy as mb


def literal_bridge(masks, class_ids):
    """build/mask_ori.py:87-124, literally: maskNP[maskOri != 0] = 255, then sorted(results, key=lambda x: np.sum(x[0]), reverse=True)."""
    results = []
    for maskOri, c in zip(masks, class_ids):
        maskNP = np.zeros(maskOri.shape, np.uint8)
        maskNP[maskOri != 0] = 255
        results.append((maskNP, int(c)))
    results = sorted(results, key=lambda x: np.sum(x[0]), reverse=True)
    if not results:
        return np.zeros((0,) + masks.shape[1:], np.uint8), np.zeros(0, np.int32)
    return np.stack([r[0] for r in results]), np.asarray([r[1] for r in results], np.int32)


def _oracle_clean(orc, masks):
    m = np.ascontiguousarray(masks).copy()
    L = orc.lib()
    L.orc_mask_clean_overlap.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.orc_mask_clean_overlap(orc.ptr(m), m.shape[0], m.shape[2], m.shape[1])
    return m


def _random_case(rng, n, H, W):
    """n Bernoulli fields of mixed densities, with ties: some masks are pixel permutations of others (equal areas), some are empty."""
    dens = rng.choice([0.0, 0.01, 0.3, 0.5, 0.99, 1.0], n)
    bm = rng.random((n, H, W)) < dens[:, None, None]
    for k in range(2, n, 3):
        bm[k] = np.roll(bm[k - 2], 5, axis=1)
    return bm, rng.integers(0, 80, n).astype(np.int32)


def test_statement_equals_the_literal_bridge_and_the_oracle_clean(orc):
    rng = np.random.default_rng(5)
    for n, H, W in ((0, 12, 16), (1, 12, 16), (2, 12, 16), (7, 24, 20), (12, 16, 32), (40, 8, 12)):
        bm, cls = _random_case(rng, n, H, W)
        for fmt in ("bool", "uint8", "float32"):
            if fmt == "bool":
                raw, thr = bm, 0.5
            elif fmt == "uint8":
                raw, thr = np.where(bm, rng.integers(1, 256, bm.shape), 0).astype(np.uint8), 0.5
            else:
                thr = 0.7
                raw = np.where(bm, np.nextafter(np.float32(thr), np.float32(2)), np.float32(thr)).astype(np.float32)
            ori, clean, order, out_cls = mb.bridge_masks(raw, cls, thr)
            want_ori, want_cls = literal_bridge(bm, cls)
            assert ori.dtype == np.uint8 and clean.dtype == np.uint8 and order.dtype == np.int32 and out_cls.dtype == np.int32
            assert np.array_equal(ori, want_ori) and np.array_equal(out_cls, want_cls), (n, fmt)
            assert sorted(order.tolist()) == list(range(n)) and np.array_equal(cls[order], out_cls)
            area = bm.sum(axis=(1, 2))[order]
            assert (np.diff(area) <= 0).all()
            assert all(order[k] < order[k + 1] for k in range(n - 1) if area[k] == area[k + 1])      # stable
            if n:
                assert np.array_equal(clean, _oracle_clean(orc, ori)), (n, fmt)
        if n >= 7:
            assert len(set(area.tolist())) < n and (clean != ori).any()
        assert np.array_equal(mb.bridge_masks(bm[:, None], cls)[1], mb.bridge_masks(bm, cls)[1])     # [N,1,H,W]


def test_inside_rule_at_its_edges():
    f = np.float32
    t07 = f(0.7)
    v = np.array([t07, np.nextafter(t07, f(2)), np.nextafter(t07, f(-2)), np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45], np.float32)
    assert mb.inside(v, 0.7).tolist() == [False, True, False, False, True, False, False, False, False, False]
    assert mb.inside(v, 0.0).tolist() == [True, True, True, False, True, False, False, False, True, False]      # -0.0 > 0 is false, a denormal is above 0
    assert mb.inside(v, -1.0).tolist() == [True, True, True, False, True, False, True, True, True, True]
    assert not mb.inside(v, np.inf).any() and not mb.inside(v, np.nan).any()
    assert mb.inside(np.array([0, 1, 128, 255], np.uint8)).tolist() == [False, True, True, True]
    assert mb.inside(np.array([False, True])).tolist() == [False, True]


def test_header_declares_and_binding_covers_the_entry():
    import instancefusion_amd as m

    header = open(m.HEADER_PATH).read()
    decl = re.search(r"\bint\s+ifx_ingest_masks\s*\(([^;]*)\);", header)
    assert decl and "ifx_ingest_masks" in m.exported_symbols()
    assert len(m._SIGS["ifx_ingest_masks"][1]) == decl.group(1).count(",") + 1
    assert callable(m.InstanceFusion.ingest_masks)
