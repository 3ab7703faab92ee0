"""Numpy restatement of the id-image translation of a deferred segmentation call (ifx_process_segmentation_deferred, k_seg_translate): the id image of the frame
a snapshot was taken at, named by creation numbers, re-addressed in the slots of a later, compacted map.  Shared by tests/test_seg_deferred_cpu.py and
tests/test_gpu_seg_deferred.py."""
import numpy as np


def translate_ids(ids_then, seq_then, seq_now):
    """ids_then: int32 id image (slots of the compacted map it was rendered on, 0 = no surfel); seq_then / seq_now: ascending creation numbers of the live surfels in
    download order, then and now.  A pixel keeps its surfel if the creation number is still in seq_now; a number that is gone reads 0, and so does the surfel that
    now sits at index 0 (the reference's "surfel 0" is never voted for)."""
    ids_then = np.asarray(ids_then)
    seq_then = np.asarray(seq_then, np.uint32)
    seq_now = np.asarray(seq_now, np.uint32)
    out = np.zeros(ids_then.shape, np.int32)
    has = (ids_then > 0) & (ids_then < seq_then.size)
    if not has.any() or seq_now.size == 0:
        return out
    want = seq_then[ids_then[has]]
    j = np.searchsorted(seq_now, want)
    found = (j < seq_now.size) & (seq_now[np.minimum(j, seq_now.size - 1)] == want)
    out[has] = np.where(found, j, 0).astype(np.int32)      # missing -> 0; index 0 -> 0 by its value
    return out
