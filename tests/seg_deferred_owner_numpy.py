"""Numpy statement of the per-rank id-image translation of a deferred segmentation call on a spatially sharded map (ifx_owner_segmentation_begin_deferred*): the
replicated id image a ticket pinned -- creation numbers, 0 = no surfel -- re-addressed in the slots one rank's shard has when the masks arrive.  Written from the
rule in include/ifx_c_api.h, not from the kernel.  Shared by tests/test_seg_deferred_owner_cpu.py and tests/test_gpu_owner_seg_deferred.py."""
import numpy as np


def translate_ids_owner(pinned, seq_now, alive_now, surfel0):
    """pinned: the ticket's id image as creation numbers (int32 or uint32 bits, 0 = no surfel); seq_now: this rank's creation numbers in slot order, ascending,
    tombstones included; alive_now: per slot, tm.y > DEAD_TIME; surfel0: today's "surfel 0", the lowest live creation number of ANY rank (0 under the test switch
    own_first_live = 0: no id image names creation number 0).
    A pixel keeps its surfel on this rank if the number is still stored here, the slot is alive, and the number is not surfel0.  Returns the int32 image the call
    body reads: slot + 1 where the pixel keeps its surfel, 0 = no surfel of this rank."""
    want = np.ascontiguousarray(pinned).view(np.uint32) if np.asarray(pinned).dtype == np.int32 else np.asarray(pinned, np.uint32)
    seq_now = np.asarray(seq_now, np.uint32)
    alive_now = np.asarray(alive_now, bool)
    out = np.zeros(want.shape, np.int32)
    if seq_now.size == 0:
        return out
    j = np.minimum(np.searchsorted(seq_now, want), seq_now.size - 1)
    keep = (want != 0) & (seq_now[j] == want) & alive_now[j] & (want != np.uint32(surfel0))
    out[keep] = (j[keep] + 1).astype(np.int32)
    return out


def lost_owner(pinned, seq_then, seq_now, alive_now, surfel0):
    """pixels whose surfel this rank owned at the snapshot (seq_then: its creation numbers then) and that read 0 now: what ifx_segmentation_snapshot_stats reports
    as `lost` on a sharded ticket"""
    want = np.ascontiguousarray(pinned).view(np.uint32) if np.asarray(pinned).dtype == np.int32 else np.asarray(pinned, np.uint32)
    mine = (want != 0) & np.isin(want, np.asarray(seq_then, np.uint32))
    return int((mine & (translate_ids_owner(pinned, seq_now, alive_now, surfel0) == 0)).sum())
