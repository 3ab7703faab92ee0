"""Deferred segmentation without a GPU: the five C-ABI entries are declared in the header and bound by the Python package, and the numpy translation helper the
GPU tests compare against does what its docstring says on a hand-made pair of creation-number lists."""
import re

import numpy as np

from seg_deferred_numpy import translate_ids

ENTRIES = ("ifx_segmentation_snapshot", "ifx_process_segmentation_deferred", "ifx_process_segmentation_deferred_device", "ifx_segmentation_snapshot_release",
           "ifx_segmentation_snapshot_stats")


def test_header_declares_and_binding_covers_the_entries():
    import instancefusion_amd as m

    header = open(m.HEADER_PATH).read()
    bound = m.exported_symbols()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*ifx_t\s*\*\s*h\b", header), name
        assert name in bound, name
    # argument counts of the binding follow the header's declarations
    for name in ENTRIES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header).group(1)
        assert len(m._SIGS[name][1]) == decl.count(",") + 1, name
    for meth in ("snapshot", "process_segmentation_deferred", "process_segmentation_deferred_device", "release_snapshot", "snapshot_stats"):
        assert callable(getattr(m.InstanceFusion, meth)), meth


def test_translation_helper_on_a_hand_made_pair():
    seq_then = np.array([3, 5, 6, 8, 9], np.uint32)
    # surfel 3 stays at index 0 (first live: never voted for), 5 is unmoved at index 1, 6 was removed, 8 and 9 moved down by one, 12 is new
    seq_now = np.array([3, 5, 8, 9, 12], np.uint32)
    ids = np.array([[0, 1, 2, 3, 4], [4, 3, 2, 1, 0]], np.int32)   # id 0 = no surfel (the first live surfel is never drawn)
    t = translate_ids(ids, seq_then, seq_now)
    assert t.dtype == np.int32 and t.shape == ids.shape
    assert t.tolist() == [[0, 1, 0, 2, 3], [3, 2, 0, 1, 0]]
    # surfel 3 removed as well: 5 becomes the first live surfel and reads 0 from now on; nothing names the new surfel
    seq_now2 = np.array([5, 8, 9, 12], np.uint32)
    t2 = translate_ids(ids, seq_then, seq_now2)
    assert t2.tolist() == [[0, 0, 0, 1, 2], [2, 1, 0, 0, 0]]
    assert not (t2 == 3).any()
    # nothing changed: the identity (except that id 0 stays 0); an empty map: all zero
    assert np.array_equal(translate_ids(ids, seq_then, seq_then), ids)
    assert not translate_ids(ids, seq_then, np.zeros(0, np.uint32)).any()
