"""The ten segmentation entries of the C ABI refuse alike: a table over ifx_process_segmentation{,_device,_rois,_detections}, their four deferred twins and the
two stage entries (ifx_ingest_masks, ifx_paste_roi_masks).  Every case is refused before anything is enqueued; the return code and the entry's own name at the start
of ifx_last_error are asserted.  Codes as the entries have always returned them: IFX_E_INVALID (-1) for arguments and unknown tickets, IFX_E_STATE (-4) by mode.
The two host entries are held to the family's wording ("<entry>: n must be 0 .. 256", "<entry>: null masks or class ids").

The detection entries count rows, not masks: R may be 0 .. 1024 (257 rows are a valid call), so their over-limit case is R = 1025, and their ROI size is M.
Only pointers an entry requires are tried as null: the host frame, the stream, d_count, d_class_map and the outputs of the stage entries are optional."""
import ctypes as C

import numpy as np
import pytest

from conftest import SMALL

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4
UNKNOWN_TICKET = 12345
NMAX = 257      # the buffers hold what the largest refused count would read, were it not refused
RMAX = 1025


@pytest.fixture(scope="module")
def bufs():
    """host and device buffers every case points at (never read: each case is refused at entry)"""
    import torch

    import instancefusion_amd as m

    W, H = SMALL["w"], SMALL["h"]
    t = dict(
        d_masks=torch.zeros((NMAX, H, W), dtype=torch.uint8, device="cuda"),
        d_rois=torch.zeros((NMAX, 65, 65), dtype=torch.float32, device="cuda"),
        d_boxes=torch.zeros((RMAX, 4), dtype=torch.float32, device="cuda"),
        d_cls=torch.zeros(NMAX, dtype=torch.int32, device="cuda"),
        d_logits=torch.zeros((RMAX, 1, 65, 65), dtype=torch.float32, device="cuda"),
        d_scores=torch.zeros(RMAX, dtype=torch.float32, device="cuda"),
        d_labels=torch.zeros(RMAX, dtype=torch.int64, device="cuda"),
    )
    torch.cuda.synchronize()
    h_masks, h_cls = np.zeros((NMAX, H, W), np.uint8), np.zeros(NMAX, np.int32)
    p = m.MaskHeadParams(0.7, W, H, W, H, 1)
    v = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    v.update(h_masks=h_masks.ctypes.data_as(C.c_void_p), h_cls=h_cls.ctypes.data_as(C.c_void_p), params=C.pointer(p))
    return v, (t, h_masks, h_cls, p)   # (the second member keeps the memory alive)


# entry -> its arguments behind the handle, in order: (name, default); a default that is a string names a buffer of `bufs`
_IMAGE = [("masks", "d_masks"), ("format", 0), ("threshold", 0.5), ("cls", "d_cls"), ("n", 1)]
_ROIS = [("rois", "d_rois"), ("roi_size", 28), ("boxes", "d_boxes"), ("threshold", 0.5), ("cls", "d_cls"), ("n", 1)]
_DET = [("logits", "d_logits"), ("boxes", "d_boxes"), ("scores", "d_scores"), ("labels", "d_labels"), ("count", None), ("class_map", None), ("n", 1), ("C", 1), ("roi_size", 28),
        ("params", "params"), ("threshold", 0.5)]
_CALL = [("frame", 100), ("flags", 0), ("stream", None)]
_OUT = [("stream", None), ("out_ori", None), ("out_clean", None), ("out_order", None), ("out_cls", None)]
_TICKET = [("ticket", UNKNOWN_TICKET)]
_HOST = [("masks", "h_masks"), ("cls", "h_cls"), ("n", 1), ("frame", 100), ("flags", 0)]
ENTRIES = {
    "ifx_process_segmentation": [("rgb", None), ("depth", None)] + _HOST,
    "ifx_process_segmentation_device": _IMAGE + _CALL,
    "ifx_process_segmentation_rois": _ROIS + _CALL,
    "ifx_process_segmentation_detections": _DET + _CALL + [("out_kept", None)],
    "ifx_process_segmentation_deferred": _TICKET + _HOST,
    "ifx_process_segmentation_deferred_device": _TICKET + _IMAGE + _CALL,
    "ifx_process_segmentation_deferred_rois": _TICKET + _ROIS + _CALL,
    "ifx_process_segmentation_deferred_detections": _TICKET + _DET + _CALL + [("out_kept", None)],
    "ifx_ingest_masks": _IMAGE + _OUT,
    "ifx_paste_roi_masks": _ROIS + _OUT,
}
REQUIRED = {"masks", "cls", "rois", "boxes", "logits", "scores", "labels", "params"}   # the pointers an entry refuses as null


def _argument_cases(name):
    """(what, overrides) of every argument refusal of one entry"""
    names = [a for a, _ in ENTRIES[name]]
    det = "logits" in names
    cases = [("count over the limit", dict(n=RMAX if det else NMAX)), ("count -1", dict(n=-1))]
    cases += [(f"null {a}", {a: None}) for a in names if a in REQUIRED]
    if "format" in names:
        cases.append(("unknown mask format", dict(format=7)))
    if "roi_size" in names:
        cases += [("roi_size 0", dict(roi_size=0)), ("roi_size 65", dict(roi_size=65))]
    return cases


def _call(L, handle, bufs, name, **over):
    args = []
    for a, default in ENTRIES[name]:
        x = over.get(a, default)
        args.append(bufs[x] if isinstance(x, str) else x)
    return getattr(L, name)(handle, *args)


def _refused(L, handle, bufs, name, what, code, **over):
    L.ifx_set_option(handle, b"no_such_option_of_the_refusal_table", 0)   # (another failure's message in between: a refusal that sets none would show it)
    r = _call(L, handle, bufs, name, **over)
    err = L.ifx_last_error(handle).decode()
    print(f"{name:46s} {what:24s} -> {r}  {err}")
    assert r == code, (name, what, r, err)
    assert err.startswith(name + ": "), (name, what, err)


def test_every_entry_refuses_under_its_own_name(small_stream, bufs):
    import torch

    import instancefusion_amd as ifx

    v, _keep = bufs
    L = ifx.lib()
    g = ifx.ElasticFusion(**SMALL, max_surfels=100000)                       # no frame processed
    e = ifx.ElasticFusion(**SMALL, max_surfels=100000, n_ranks=-1, rank=0)   # an emulated sharded map
    try:
        for name in ENTRIES:
            for what, over in _argument_cases(name):
                _refused(L, g.handle, v, name, what, INVALID, **over)
            if "ticket" in [a for a, _ in ENTRIES[name]]:
                _refused(L, g.handle, v, name, "unknown ticket", INVALID)
                _refused(L, e.handle, v, name, "ticket on a sharded map", STATE, ticket=0)
            elif name != "ifx_process_segmentation":   # (the resident host entry has no refusal by mode: the owners' call is built on its schedule)
                _refused(L, e.handle, v, name, "sharded map", STATE)
        # the refusals left the handle and its event pool usable: three frames, then a valid device call
        from instancefusion_amd import synth

        st = small_stream
        for i in range(3):
            g.processFrame(st["rgb"][i], st["depth"][i])
        mk, cl = synth.canned_masks(st["obj"][2], st["scene"])
        d_mk = torch.from_numpy(np.ascontiguousarray(mk, np.uint8)).cuda()
        torch.cuda.synchronize()
        ifx.InstanceFusion(g).process_segmentation_device(d_mk, cl, 2)
    finally:
        e.close()
        g.close()
