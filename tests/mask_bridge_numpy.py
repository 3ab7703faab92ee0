"""The ingestion of ifx_process_segmentation_device / ifx_ingest_masks as numpy: what the reference's Mask-RCNN bridge hands over (build/mask_ori.py:87-124 --
binarised to 0/255, then a STABLE sort by area, descending) and the overlap clean that follows it (maskCleanOverlapKernel, IF/Core/InstanceFusionCuda.cu:118-131:
a pixel stays only in the last mask of the sorted order that holds it).  No GPU, no library: tests/test_mask_bridge_cpu.py pins it, the GPU tests compare with it."""
import numpy as np


def inside(masks, thr=0.5):
    """bool / uint8: non-zero.  float32: > float32(thr); NaN is outside (every comparison with NaN is false, and so is every comparison with a NaN threshold)."""
    masks = np.asarray(masks)
    if masks.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return masks > np.float32(thr)
    if masks.dtype in (np.bool_, np.uint8):
        return masks != 0
    raise TypeError(f"masks: dtype {masks.dtype}")


def bridge_masks(masks, class_ids, thr=0.5):
    """masks [N,H,W] or [N,1,H,W] (bool, uint8 or float32), N class ids -> (ori uint8 [N,H,W] 0/255 in sorted order, clean uint8 [N,H,W], order int32 [N] of input
    indices, class ids int32 [N] in sorted order)."""
    masks = np.asarray(masks)
    if masks.ndim == 4:
        assert masks.shape[1] == 1
        masks = masks[:, 0]
    n = masks.shape[0]
    cls = np.asarray(class_ids).astype(np.int32).reshape(-1)
    assert cls.shape[0] == n
    ins = inside(masks, thr)
    area = ins.sum(axis=(1, 2)).astype(np.int64)
    order = np.argsort(-area, kind="stable").astype(np.int32)
    ori = np.where(ins[order], np.uint8(255), np.uint8(0)).astype(np.uint8).reshape((n,) + masks.shape[1:])
    later = np.zeros(masks.shape[1:], bool)          # pixels held by a mask later in the sorted order
    clean = np.zeros_like(ori)
    for s in range(n - 1, -1, -1):
        here = ori[s] != 0
        clean[s] = np.where(here & ~later, np.uint8(255), np.uint8(0))
        later |= here
    return ori, clean, order, cls[order]
