"""The record of the sharded segmentation call's device forms (ifx_owner_segmentation_begin_device / _rois / _detections, include/ifx_c_api.h) as numpy: what
the detector's rank packs and one broadcast carries, and the ingest from its bit form.  int32 words:

  header[8]  magic, form (1 image bits, 2 ROI masks), n, M, P, max_n, 0, 0
  cls[max_n] the caller's class ids in the caller's order, rows >= n zero
  form 2     boxes f32[max_n][4], rois f32[max_n][M][M], rows >= n zero
  form 1     bits u32[max_n][ceil(P / 32)]: bit b of word j of mask m = pixel 32 j + b, binarised by the bridge's rule; bits past P and rows >= n zero

No GPU, no library: tests/test_owner_seg_record_cpu.py pins it against mask_bridge_numpy, tests/test_gpu_owner_seg_device.py compares the library's record with it."""
import numpy as np

import mask_bridge_numpy as mb

MAGIC = 0x49465852
HDR = 8


def words_per_mask(P):
    return (P + 31) // 32


def record_words(form, max_n, M, P):
    return HDR + max_n + (max_n * 4 + max_n * M * M if form == 2 else max_n * words_per_mask(P))


def _head(form, n, M, P, max_n, class_ids):
    cls = np.zeros(max_n, np.int32)
    cls[:n] = np.asarray(class_ids).astype(np.int32).reshape(-1)
    return np.concatenate([np.array([MAGIC, form, n, M, P, max_n, 0, 0], np.int32), cls])


def pack_bits(masks, thr=0.5):
    """masks [N,H,W] (bool, uint8 or float32) -> uint32 [N, ceil(P / 32)], little-endian bit order within a word"""
    masks = np.asarray(masks)
    n = masks.shape[0]
    ins = mb.inside(masks, thr).reshape(n, -1)
    P = ins.shape[1]
    padded = np.zeros((n, words_per_mask(P) * 32), np.uint8)
    padded[:, :P] = ins
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4")


def record_image(masks, class_ids, max_n, thr=0.5):
    """form 1 -> int32 [record_words]"""
    masks = np.asarray(masks)
    if masks.ndim == 4:
        masks = masks[:, 0]
    n, P = masks.shape[0], int(masks.shape[1] * masks.shape[2])
    assert n <= max_n
    bits = np.zeros((max_n, words_per_mask(P)), np.uint32)
    if n:
        bits[:n] = pack_bits(masks, thr)
    return np.concatenate([_head(1, n, 0, P, max_n, class_ids), bits.reshape(-1).view(np.int32)])


def record_rois(roi_masks, boxes, class_ids, max_n, P):
    """form 2 -> int32 [record_words]"""
    roi_masks = np.asarray(roi_masks, np.float32)
    if roi_masks.ndim == 4:
        roi_masks = roi_masks[:, 0]
    n, M = roi_masks.shape[0], int(roi_masks.shape[-1])
    assert n <= max_n
    bx = np.zeros((max_n, 4), np.float32)
    rm = np.zeros((max_n, M, M), np.float32)
    bx[:n] = np.asarray(boxes, np.float32).reshape(n, 4)
    rm[:n] = roi_masks
    return np.concatenate([_head(2, n, M, P, max_n, class_ids), bx.reshape(-1).view(np.int32), rm.reshape(-1).view(np.int32)])


def parse_header(rec):
    magic, form, n, M, P, max_n, z0, z1 = (int(v) for v in rec[:HDR])
    assert magic == MAGIC and z0 == 0 and z1 == 0
    return form, n, M, P, max_n


def ingest_bits(rec, shape):
    """The ingest of a form 1 record: areas by popcount, mask_bridge_numpy's order (stable, by area, descending), the masks in that order and the overlap clean.
    -> (ori uint8 [n,H,W] 0/255, clean, order int32 [n], class ids int32 [n] in sorted order), as mask_bridge_numpy.bridge_masks returns them."""
    form, n, M, P, max_n = parse_header(rec)
    assert form == 1 and P == shape[0] * shape[1]
    NW = words_per_mask(P)
    cls = np.asarray(rec[HDR:HDR + n], np.int32)
    bits = np.ascontiguousarray(rec[HDR + max_n:HDR + max_n + max_n * NW]).view(np.uint32).reshape(max_n, NW)[:n]
    unpacked = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little") if n else np.zeros((0, NW * 32), np.uint8)
    area = unpacked.sum(axis=1).astype(np.int64)            # popcounts of the words
    order = np.argsort(-area, kind="stable").astype(np.int32)
    ori = (unpacked[order, :P] * np.uint8(255)).astype(np.uint8).reshape((n,) + tuple(shape))
    later = np.zeros(shape, bool)
    clean = np.zeros_like(ori)
    for s in range(n - 1, -1, -1):
        here = ori[s] != 0
        clean[s] = np.where(here & ~later, np.uint8(255), np.uint8(0))
        later |= here
    return ori, clean, order, cls[order]
