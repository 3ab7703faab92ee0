"""What the GPU tests of the Keras detector's three layers share (test_gpu_keras_proposals.py, test_gpu_pyramid_roi_align.py, test_gpu_keras_detections.py): the raw
C calls with every output between prefilled guard bands, and the bit-for-bit comparison with the numpy statement (tests/keras_layers_numpy.py).  A NaN coordinate
is compared as a NaN: its payload is not part of the rule."""
import ctypes as C

import numpy as np

import keras_layers_numpy as kl

F = np.float32
GUARD = 64
E_INVALID = -1
Q = dict(w=160, h=120, fx=132.0, fy=132.0, cx=80.0, cy=60.0)


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_floats(got, ref):
    """bit for bit, a NaN against a NaN"""
    got, ref = np.ascontiguousarray(got, F), np.ascontiguousarray(ref, F)
    nan = np.isnan(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), nan), int((np.isnan(got) != nan).sum())
    bad = bits(got)[~nan] != bits(ref)[~nan]
    assert not bad.any(), int(bad.sum())


def guarded(count, dtype, fill):
    """a device buffer of `count` elements between two guard bands: (buffer, pointer to the payload)"""
    import torch

    b = torch.full((2 * GUARD + count,), fill, dtype=dtype, device="cuda")
    return b, C.c_void_p(b.data_ptr() + GUARD * b.element_size())


def payload(buf, fill):
    """the payload of a guarded buffer on the host; the guard bands must be as they were"""
    h = buf.cpu().numpy()
    assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), "a guard band was written"
    return h[GUARD:-GUARD]


def stream_ptr(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def proposal_params(ifx, image_shape, pre, count, thr, std_dev=kl.STD_DEV):
    p = ifx.KerasProposalParams()
    p.pre_nms_limit, p.proposal_count, p.nms_threshold = int(pre), int(count), float(thr)
    p.std_dev[:] = [float(v) for v in std_dev]
    p.image_h, p.image_w = int(image_shape[0]), int(image_shape[1])
    return p


def raw_proposals(ifx, ef, d_probs, d_bbox, d_anc, image_shape, pre, count, thr, std_dev=kl.STD_DEV, index=True, stream=None):
    """ifx_keras_proposals itself: the guarded torch buffers (read them with read_proposals once the stream is done)"""
    import torch

    n = int(d_probs.shape[0])
    bufs = [guarded(4 * count, torch.float32, -7.5), guarded(count, torch.int64, -77), guarded(1, torch.int32, -77)]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())                                # (the fills above are on the current stream)
    p = proposal_params(ifx, image_shape, pre, count, thr, std_dev)
    r = ef.L.ifx_keras_proposals(ef.handle, C.c_void_p(d_probs.data_ptr()), C.c_void_p(d_bbox.data_ptr()), C.c_void_p(d_anc.data_ptr()), n, C.byref(p), bufs[0][1],
                                 bufs[1][1] if index else None, bufs[2][1], stream_ptr(stream))
    assert r == 0, ef.L.ifx_last_error(ef.handle)
    return [b for b, _ in bufs]


def read_proposals(bufs, count):
    return payload(bufs[0], -7.5).reshape(count, 4), payload(bufs[1], -77), int(payload(bufs[2], -77)[0])


def proposals_equal(got, ref, count):
    boxes, index, c = got
    pb, pi, rc = kl.proposals_padded(ref, count)
    assert c == rc, (c, rc)
    if index is not None:
        assert np.array_equal(index, pi), int((index != pi).sum())
    same_floats(boxes, pb)


def detection_params(ifx, window, image_shape, min_confidence, thr, max_instances, std_dev=kl.STD_DEV):
    p = ifx.KerasDetectionParams()
    p.std_dev[:] = [float(v) for v in std_dev]
    p.min_confidence, p.nms_threshold, p.max_instances = float(min_confidence), float(thr), int(max_instances)
    p.image_h, p.image_w = int(image_shape[0]), int(image_shape[1])
    p.window[:] = [float(v) for v in window]
    return p


def raw_detections(ifx, ef, d_rois, d_probs, d_deltas, window, image_shape, min_confidence, thr, max_instances, norm=True, index=True, stream=None):
    """ifx_keras_detections itself: the guarded torch buffers (detections, boxes_norm, index, count)"""
    import torch

    R, Cn = (int(v) for v in d_probs.shape)
    M = max_instances
    bufs = [guarded(6 * M, torch.float32, -7.5), guarded(4 * M, torch.float32, -7.5), guarded(M, torch.int64, -77), guarded(1, torch.int32, -77)]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    p = detection_params(ifx, window, image_shape, min_confidence, thr, M)
    r = ef.L.ifx_keras_detections(ef.handle, C.c_void_p(d_rois.data_ptr()), C.c_void_p(d_probs.data_ptr()), C.c_void_p(d_deltas.data_ptr()), R, Cn, C.byref(p),
                                  bufs[0][1], bufs[1][1] if norm else None, bufs[2][1] if index else None, bufs[3][1], stream_ptr(stream))
    assert r == 0, ef.L.ifx_last_error(ef.handle)
    return [b for b, _ in bufs]


def read_detections(bufs, M):
    return payload(bufs[0], -7.5).reshape(M, 6), payload(bufs[1], -7.5).reshape(M, 4), payload(bufs[2], -77), int(payload(bufs[3], -77)[0])


def detections_equal(got, ref, M, norm=True, index=True):
    det, nb, idx, c = got
    pd, pn, pi, rc = kl.detections_padded(ref, M)
    assert c == rc, (c, rc)
    same_floats(det, pd)
    if norm:
        same_floats(nb, pn)
    else:
        assert (nb == -7.5).all()
    if index:
        assert np.array_equal(idx, pi)
    else:
        assert (idx == -77).all()


def proposal_case(seed, n, image=1024, quantise=0):
    """(probs [n,2], bbox [n,4], anchors [n,4] pixels): anchors of 16 .. 512 pixels in clusters around and across a square image, N(0, 0.5) deltas; the background column is larger
    than the foreground one everywhere, so a read of the wrong column cannot pass; quantise > 0: that many distinct scores (thousands of ties)"""
    rng = np.random.default_rng(seed)
    fg = rng.random(n).astype(F)
    if quantise:
        fg = (np.floor(fg * quantise) / quantise).astype(F)
    probs = np.stack([fg + F(1.5), fg], axis=1).astype(F)
    centres = rng.uniform(-32, image + 32, (max(n // 96, 8), 2))             # a hundred anchors around each centre: most of them suppress one another
    g = rng.integers(0, centres.shape[0], n)
    c = centres[g] + rng.uniform(-6, 6, (n, 2))
    hw = np.exp(rng.uniform(np.log(16), np.log(512), (centres.shape[0], 2)))[g] * rng.uniform(0.9, 1.1, (n, 2))
    anchors = np.concatenate([c - hw / 2, c + hw / 2], axis=1).astype(F)
    bbox = (rng.standard_normal((n, 4)) * 0.5).astype(F)
    return probs, bbox, anchors
