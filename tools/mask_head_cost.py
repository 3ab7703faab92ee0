"""What the stretch between the mask head's last convolution and the ROI paste costs on the GPU (ifx_mask_head_select, two launches) beside the reference's
formulation in stock PyTorch on the same inputs and the same build: x.sigmoid() over all [R, C, M, M] logits, [arange, labels], the box multiply
(maskrcnn_benchmark/modeling/roi_heads/mask_head/inference.py:27-61, structures/bounding_box.py:91-127), then scores > t -> nonzero, the gathers, sort, the gathers
again (demo/predictor.py:224-243).  Workload: R = 100, C = 81, M = 28 on a 640 x 480 frame (the network's input 1067 x 800), with about 10 and about 60 rows above
0.7.  Per figure: HIP-event time of the whole call on its stream and the host time until the call returns; the two paths are run alternately, `rounds` rounds of
`calls` calls each, and the median of every round and the median of those medians are printed.  The results of the two paths are compared first (rows, order and
class ids equal; probabilities within a few ulp: torch's sigmoid is another function).  Launches: ours from the library's kernel timing; the stock path's are
counted as the tensor operations it issues (each is one launch or more; nonzero is several and makes the host wait).

    python tools/mask_head_cost.py [calls] [rounds]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: libifx.so binds to the HIP runtime torch ships)
import numpy as np  # noqa: E402

import instancefusion_amd as ifx  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
R, CN, M = 100, 81, 28
IN_SIZE, OUT_SIZE, T = (1067, 800), (640, 480), 0.7
ef = ifx.ElasticFusion(w=640, h=480, fx=528.0, fy=528.0, cx=320.0, cy=240.0, max_surfels=100000)
rng = np.random.default_rng(1)


def timed(fn, reps):
    """HIP-event time of fn() on the current stream and the host time until it returns: medians in us"""
    dev, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        b.record()
        b.synchronize()
        dev.append(a.elapsed_time(b) * 1e3); host.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.median(host))


STOCK_OPS = 15      # sigmoid, arange, index, multiply, compare, nonzero, four gathers, sort, four gathers


def stock(x, boxes, scores, labels, ratio):
    prob = x.sigmoid()
    own = prob[torch.arange(x.shape[0], device=x.device), labels][:, None]
    bx = boxes * ratio
    keep = torch.nonzero(scores > T).squeeze(1)                          # the host waits here for the count
    bx, sc, lb, own = bx[keep], scores[keep], labels[keep], own[keep]
    _, order = sc.sort(0, descending=True)
    return own[order], bx[order], lb[order], sc[order]


print(f"mask_head_cost: {torch.cuda.get_device_name(0)}, R = {R}, C = {CN}, M = {M}, {rounds} alternating rounds of {calls} calls, medians")
x = torch.randn(R, CN, M, M, device="cuda") * 4.0
x0 = rng.uniform(0, IN_SIZE[0] * 0.8, R); y0 = rng.uniform(0, IN_SIZE[1] * 0.8, R)
boxes = torch.from_numpy(np.stack([x0, y0, x0 + rng.uniform(8, 200, R), y0 + rng.uniform(8, 150, R)], axis=1).astype(np.float32)).cuda()
labels = torch.from_numpy(rng.integers(1, CN, R).astype(np.int64)).cuda()
ratio = torch.tensor([OUT_SIZE[0] / IN_SIZE[0], OUT_SIZE[1] / IN_SIZE[1]] * 2, dtype=torch.float32, device="cuda")
for above in (10, 60):
    s = rng.uniform(0.05, 0.69, R)
    s[rng.permutation(R)[:above]] = rng.uniform(0.71, 0.999, above)
    scores = torch.from_numpy(s.astype(np.float32)).cuda()
    one = lambda: ef.mask_head_select(x, boxes, scores, labels, IN_SIZE, OUT_SIZE, T, True, padded=True)
    cut = lambda: ef.mask_head_select(x, boxes, scores, labels, IN_SIZE, OUT_SIZE, T, True)
    ref = lambda: stock(x, boxes, scores, labels, ratio)
    m, b, c, rows, kept = one()
    rm, rb, rl, rs = ref()
    torch.cuda.synchronize()
    k = int(kept.item())
    same_rows = bool(torch.equal(scores[rows[:k].long()], rs)) and bool(torch.equal(c[:k].long(), rl))
    ulp = float(((m[:k] - rm[:, 0]).abs() / torch.from_numpy(np.spacing(rm[:, 0].cpu().numpy())).cuda()).max()) if k else 0.0
    print(f"  {k} rows above {T}: scores in order and class ids equal to the stock path's: {same_rows}; boxes equal: {bool(torch.equal(b[:k], rb))}; probabilities "
          f"within {ulp:.1f} ulp of torch's sigmoid; sigmoids evaluated: {k * M * M} against {R * CN * M * M}")
    for _ in range(3):
        one(); cut(); ref()
    torch.cuda.synchronize()
    res = {"one": [], "cut": [], "ref": []}
    for _ in range(rounds):
        res["one"].append(timed(one, calls))
        res["cut"].append(timed(cut, calls))
        res["ref"].append(timed(ref, calls))
    for name, key, launches, syncs in (("mask_head_select(padded=True)", "one", "2", 0), ("mask_head_select, cut to kept  ", "cut", "2", 1),
                                       ("stock PyTorch                 ", "ref", f"{STOCK_OPS} tensor operations", 1)):
        dev, host = [v[0] for v in res[key]], [v[1] for v in res[key]]
        print(f"    {name}: stream {np.median(dev):8.1f} us {[round(v, 1) for v in dev]};  the call returns after {np.median(host):8.1f} us {[round(v, 1) for v in host]};  "
              f"launches per call: {launches};  host waits per call: {syncs}")
    ef.set_option("kernel_timing", 1)
    ef.kernel_ms("__reset__")
    for _ in range(calls):
        one()
    ef.sync(); torch.cuda.synchronize()
    for kn in ("mh_select", "mh_sigmoid"):
        avg, cnt = ef.kernel_ms(kn)
        print(f"    kernel {kn} (HIP events around the launch): {avg * 1e3:.1f} us x {cnt}")
    ef.set_option("kernel_timing", 0)
ef.close()
