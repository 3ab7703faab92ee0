"""What the detector's input costs when it is made on the GPU from the resident 640x480 frame (ifx_detector_input) at min_size 512 and 800, size_divisible 32:
the kernel's HIP-event time (option kernel_timing), the host time of the enqueue-only call, the wall time to the finished tensor -- and, where Pillow is
installed, the path it replaces: Pillow's bilinear resize, the float tail and the padding in CPU torch, and the upload of the 3 x H' x W' floats.  The results of
the two paths are compared first (they are equal).

    python tools/detector_input_cost.py [calls]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402
from instancefusion_amd import synth  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 100
W, H = 640, 480
K = dict(fx=528.0, fy=528.0, cx=320.0, cy=240.0)
MEAN = (102.9801, 115.9465, 122.7717)
st = synth.make_stream(3, W, H, noise=True, **K)
ef = ifx.ElasticFusion(w=W, h=H, max_surfels=2_000_000, **K)
inst = ifx.InstanceFusion(ef)
for i in range(3):
    ef.processFrame(st["rgb"][i], st["depth"][i])
ef.sync()
rgb = st["rgb"][2]
try:
    from PIL import Image
except ImportError:
    Image = None


def cpu_path(min_size, d):
    """the reference's chain on the host with an RGB frame (transforms.py:86-90: flip and x255), then the upload"""
    ow, oh, Wp, Hp = ifx.detector_input_size(W, H, min_size, None, d)
    small = np.asarray(Image.fromarray(rgb).resize((ow, oh), Image.BILINEAR))
    t = torch.from_numpy(small).permute(2, 0, 1).float().div(255)
    t = t[[2, 1, 0]] * 255
    t.sub_(torch.tensor(MEAN)[:, None, None]).div_(torch.tensor((1.0, 1.0, 1.0))[:, None, None])
    out = torch.zeros((1, 3, Hp, Wp))
    out[0, :, :oh, :ow].copy_(t)
    return out.to("cuda")


def stats(a):
    a = np.asarray(a) * 1e6
    return f"median {np.median(a):8.1f} us  p10 {np.percentile(a, 10):8.1f}  p90 {np.percentile(a, 90):8.1f}  min {a.min():8.1f}"


print(f"detector_input_cost: {W}x{H} resident frame, size_divisible 32, flip and x255, {calls} calls per figure; Pillow {'%s' % Image.__version__ if Image else 'not installed'}")
for min_size in (512, 800):
    kw = dict(min_size=min_size, size_divisible=32, to_bgr255=True, swap_rb=True)
    out, (oh, ow) = inst.detector_input(**kw)
    torch.cuda.synchronize()
    Hp, Wp = int(out.shape[2]), int(out.shape[3])
    print(f"  min_size {min_size}: {ow}x{oh} in {Wp}x{Hp}, {out.numel() * 4 / 1e6:.2f} MB written, {W * H * 3 / 1e6:.2f} MB read")
    if Image:
        ref = cpu_path(min_size, 32)
        torch.cuda.synchronize()
        print(f"    equal to the host path: {bool(torch.equal(ref, out))}")
    for _ in range(10):
        inst.detector_input(out=out, **kw)
    torch.cuda.synchronize()
    enq, wall = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        inst.detector_input(out=out, **kw)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        enq.append(t1 - t0); wall.append(t2 - t0)
    print(f"    the call returns after          {stats(enq)}")
    print(f"    call + synchronise              {stats(wall)}")
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        inst.detector_input(out=out, **kw)
    ef.sync(); torch.cuda.synchronize()
    avg, n = ef.kernel_ms("detector_input")
    ef.set_option("kernel_timing", 0)
    print(f"    kernel detector_input (HIP events, option kernel_timing): {avg * 1e3:.1f} us x {n}")
    if Image:
        for _ in range(3):
            cpu_path(min_size, 32)
        torch.cuda.synchronize()
        host = []
        for _ in range(max(calls // 5, 10)):
            t0 = time.perf_counter()
            cpu_path(min_size, 32)
            torch.cuda.synchronize()
            host.append(time.perf_counter() - t0)
        print(f"    Pillow + CPU torch + upload     {stats(host)}   ({torch.get_num_threads()} torch threads)")
ef.close()
