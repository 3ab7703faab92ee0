"""The packed vote counters (vote_encode / vote_decode: two 16-bit counters through an int into a float) where the packing is lossy, HIP against the oracle.
A map whose votes were rewritten into those regimes -- words beyond 2^24 whose low half rounds, counters at the top of the short range, negative halves that
borrow, equal maxima in several counters, floats no encoding produces -- goes to both sides; then the same segmentation calls run on both and everything the ten
decoding kernels produce is compared after every call: votes (bit for bit), colours, labels, instance table, the rendered instance colours, the segmentation
decision.  That the calls really work in those regimes is computed from the oracle's side alone and asserted (the counts are printed)."""
import time

import numpy as np
import pytest

from conftest import SMALL

pytestmark = pytest.mark.gpu

TAG_WORD = 47
CRAFT_WORDS = 21
NW = 48                                                   # vote words per surfel: word w holds instance 2w (high half) and 2w + 1 (low half)
UNTOUCHED, CROSS, TOP, BORROW, TIE, RAW = 0, 1, 2, 3, 4, 5
NAMES = {CROSS: "crossing 2^24", TOP: "top of the range", BORROW: "borrow", TIE: "ties", RAW: "not an encoding"}
RAW_FLOATS = np.asarray([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 0.5, -0.5, 1e10], np.float32)


@pytest.fixture(scope="module")
def ifx():
    import instancefusion_amd as m

    m.lib()
    return m


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def decode(votes):
    """vote_decode of float32 words [n,48] as numpy: int32 counters [n,96] (f2i_rz: NaN -> 0, saturating, toward zero; then the two shorts)"""
    f = np.ascontiguousarray(votes, np.float32)
    with np.errstate(invalid="ignore"):
        inside = np.abs(f) < np.float32(2.0 ** 31)        # (false for NaN)
        v = np.where(inside, f, np.float32(0)).astype(np.int32)
        v[f >= np.float32(2.0 ** 31)] = np.iinfo(np.int32).max
        v[f <= np.float32(-2.0 ** 31)] = np.iinfo(np.int32).min
    out = np.zeros(f.shape[:-1] + (2 * f.shape[-1],), np.int32)
    out[..., 0::2] = v >> 16
    out[..., 1::2] = v.astype(np.int16)
    return out


def make_encoder(orc):
    L = orc.lib()
    cache = {}

    def enc(a, b):
        k = (int(a), int(b))
        if k not in cache:
            cache[k] = np.float32(L.orc_vote_encode(k[0], k[1]))
        return cache[k]

    return enc


def craft(orc, m, labels, visible, rng):
    """Rewrites m["votes"] in place: the surfels the ordinary call labelled (the calls that follow vote for them again) go into the lossy regimes, unvoted ones get
    the ties and raw floats; every crafted word that is an encoding comes from orc_vote_encode.  Returns (regime, crafted-word flags [.,48]) of the crafted surfels."""
    enc = make_encoder(orc)
    V = m["votes"]
    n = V.shape[0]
    cnt = decode(V)
    regime = np.zeros(n, np.int32)
    crafted = np.zeros((n, NW), bool)

    def put(s, w, a, b):
        V[s, w] = enc(a, b)
        crafted[s, w] = True

    # Which instance a call votes for hangs on the boxes, and those on the crafted maxima themselves: a mask that finds no instance registers the first free one.
    # So every word a few calls can reach (instances 0 .. 2 * CRAFT_WORDS - 1) of a voted surfel is put into the surfel's regime, the variants alternating by word.
    voted = np.nonzero(labels >= 0)[0]
    for k, s in enumerate(voted):
        r = (CROSS, TOP, BORROW, CROSS, RAW, CROSS, TOP, UNTOUCHED)[k % 8]
        regime[s] = r
        for w in range(CRAFT_WORDS if r != UNTOUCHED else 0):
            v = k // 8 + w
            if r == CROSS and v % 3 != 0:                 # a voted high half crosses 256, and the low half under it starts to round
                put(s, w, rng.integers(250, 263), rng.integers(1, 10))
            elif r == CROSS:                              # the mirror image: the high half is beyond 256 while the low half is voted
                hi = int(rng.integers(255, 301))
                put(s, w, hi, hi + int(rng.integers(1, 121)))
            elif r == TOP and v % 8 == 0:                 # encodes to exactly 2^31, decoded through the clamp to (32767, -1)
                put(s, w, -32768, -1)
            elif r == TOP and v % 8 == 1:                 # the short wraps: -2^31
                put(s, w, 32768, 0)
            elif r == TOP and v % 8 < 5:                  # the votes wrap the high half; the float's step is 128 here
                put(s, w, rng.integers(32700, 32768), rng.integers(0, 301))
            elif r == TOP:                                # the low half wraps and borrows
                put(s, w, rng.integers(0, 301), rng.integers(32700, 32768))
            elif r == BORROW and v % 2 == 0:              # a negative low half borrows from the high one at every decode
                put(s, w, rng.integers(1, 10), (-1, -7, -32768)[(v // 2) % 3])
            elif r == BORROW:                             # a negative high half over a voted low half
                put(s, w, (-1, -300)[(v // 2) % 2], rng.integers(1, 10))
            elif r == RAW:
                V[s, w] = RAW_FLOATS[v % len(RAW_FLOATS)]
                crafted[s, w] = True
    # unvoted surfels, under the id image and outside it: ties and raw floats
    rest = np.nonzero(labels < 0)[0]
    rest = rest[rest > 0]
    for vis in (True, False):
        pool = rest[visible[rest] == vis]
        pick = rng.choice(pool, min(len(pool), 420), replace=False)
        for k, s in enumerate(pick[:360]):
            regime[s] = TIE
            w0 = int(rng.integers(2, 8)) if k % 2 else int(rng.integers(24, 30))      # among the lower / the higher instance ids
            t = int(rng.integers(5, 41))
            kind = k % 6
            if kind == 0:      # both halves of one word
                put(s, w0, t, t)
            elif kind == 1:    # neighbouring words of one float4 (one lane of k_count_colour's group, one load)
                w0 -= w0 % 4
                put(s, w0, t, -1); put(s, w0 + 1, -1, t)
            elif kind == 2:    # words w and w + 4: neighbouring float4, two lanes
                put(s, w0, -1, t); put(s, w0 + 4, t, -1)
            elif kind == 3:    # words w and w + 16: float4 q and q + 4, the same lane's next load
                put(s, w0, t, 0); put(s, w0 + 16, 0, t)
            elif kind == 4:    # three lanes
                put(s, w0, 0, t); put(s, w0 + 4, t, 0); put(s, w0 + 8, 0, t)
            else:              # the higher index in a lower lane position: (w + 5, high) against (w, low) and a smaller count before both
                put(s, w0, t - 1, t); put(s, w0 + 5, t, t - 1)
        for k, s in enumerate(pick[360:]):
            regime[s] = RAW
            w = 4 + (k * 7) % 40
            V[s, w] = RAW_FLOATS[k % len(RAW_FLOATS)]
            crafted[s, w] = True
    m["col"][:, 1] = 0.0                                  # colours are assigned once: every scan of the calls below assigns them from the crafted votes
    # a frame may drop surfels and move the ones behind them up: every crafted surfel carries its number in the last word, as negative counters (never a maximum)
    tagged = np.nonzero(crafted.any(axis=1))[0]
    assert len(tagged) < 32000 and not crafted[:, TAG_WORD].any()
    for j, s in enumerate(tagged):
        V[s, TAG_WORD] = enc(-2, -1 - j)                  # decodes to (-3, -1 - j): the negative low half borrows
    return regime[tagged], crafted[tagged]


def find_tagged(votes, regime_t, crafted_t):
    """(regime per surfel, crafted-word flags [n,48]) of a map downloaded later, by the numbers craft() left in the last word"""
    t = decode(votes[:, TAG_WORD:TAG_WORD + 1])
    rows = np.nonzero((t[:, 0] == -3) & (t[:, 1] < 0) & (t[:, 1] >= -len(regime_t)))[0]
    j = -1 - t[rows, 1]
    assert len(set(j.tolist())) == len(j)
    regime = np.zeros(votes.shape[0], np.int32)
    crafted = np.zeros((votes.shape[0], NW), bool)
    regime[rows], crafted[rows] = regime_t[j], crafted_t[j]
    return regime, crafted, len(rows)


def one_hot_votes(votes):
    """Lossless votes that lead a call to the same decisions as `votes`: per surfel the first maximum of the positive counters (what the instance boxes read) as a
    single 1, and counter 0 kept at -1 where it is -1 (the reference's 'not projected' test)."""
    cnt = decode(votes)
    n = cnt.shape[0]
    pos = np.where(cnt > 0, cnt, 0)
    arg = pos.argmax(axis=1)
    has = pos.max(axis=1) > 0
    c = np.zeros_like(cnt)
    c[np.nonzero(has)[0], arg[has]] = 1
    c[cnt[:, 0] == -1, 0] = -1
    return (c[:, 0::2].astype(np.int64) * 65536 + c[:, 1::2]).astype(np.float32), c


class Lossless:
    """What the calls add to every counter, from the oracle's side alone: a second oracle object gets the first one's map, pose and id image before every call,
    with votes replaced by one_hot_votes (tiny counters: nothing rounds, wraps or borrows), and makes the same call; the instance table must stay the first one's."""

    def __init__(self, orc, o):
        self.p = orc.Oracle(**SMALL, max_surfels=400000)
        self.o = o
        self.total = None

    def before(self):
        m = self.o.download()
        m["votes"], self.c0 = one_hot_votes(m["votes"])
        self.p.upload(m)
        self.p.set_pose(self.o.get_pose(), self.o.tick)
        self.p.set_ids_after(self.o.image("ids_after"))

    def call(self, *a, **k):
        self.p.process_segmentation(*a, **k)
        assert np.array_equal(self.p.instance_table(), self.o.instance_table())
        inc = decode(self.p.download()["votes"]) - self.c0
        assert (inc >= 0).all()
        self.total = inc.astype(np.int64) if self.total is None else self.total + inc
        return inc

    def close(self):
        self.p.close()


def compare(g, inst, o, what, frame, scanned=True):
    """Everything the decoding kernels produce, against the oracle (scanned=False: no label scan has run on this map yet -- labels and colours are not compared)."""
    mg, mo = g.download(), o.download()
    assert np.array_equal(bits(mg["votes"]), bits(mo["votes"])), (what, "votes", np.argwhere(bits(mg["votes"]) != bits(mo["votes"]))[:5])
    assert np.array_equal(mg["col"], mo["col"]), (what, "col")
    assert not scanned or np.array_equal(inst.labels(), o.labels()), (what, "labels")
    assert np.array_equal(inst.getInstanceTable(), o.instance_table()), (what, "table")
    assert np.array_equal(inst.renderProjectMap(), o.render_project_map()), (what, "project map")
    assert inst.whetherDoSegmentation(frame) == o.should_segment(frame), (what, "should segment")
    return mo


def prepare(ifx, orc, st, seed, lossless=False):
    """test_instance_table_eviction_exact's recipe up to one ordinary call, then the rewrite on both sides and one more frame.  ifx None: the oracle's side alone."""
    from instancefusion_amd import synth

    g = inst = None
    if ifx is not None:
        g = ifx.ElasticFusion(**SMALL, max_surfels=400000)
        g.set_option("compact_every_frame", 1)
        inst = ifx.InstanceFusion(g)
    o = orc.Oracle(**SMALL, max_surfels=400000)
    rgb, dep = st["rgb"][5], st["depth"][5]
    for i in range(6):
        po = o.process_frame(st["rgb"][i], st["depth"][i])
        if g:
            g.processFrame(st["rgb"][i], st["depth"][i])

    def both_upload(m):
        o.upload(m); o.set_pose(po, o.tick)
        if g:
            g.upload(m); g.set_pose(po, o.tick)
            g.processFrame(rgb, dep, inPose=po)
        o.process_frame(rgb, dep, in_pose=po)
        if g:
            assert np.array_equal(g.image("ids_after"), o.image("ids_after"))

    m = o.download(); m["pc"][:, 3] = 20.0
    both_upload(m)
    masks, cls = synth.canned_masks(st["obj"][5], st["scene"])
    lossless = Lossless(orc, o) if lossless else None
    if lossless:
        lossless.before()
    if g:
        inst.ProcessSegmentation(rgb, dep, masks, cls, 100)
    o.process_segmentation(rgb, dep, masks, cls, 100)
    if lossless:                                          # (its table follows from the start)
        lossless.call(rgb, dep, masks, cls, 100)
        lossless.total = None
    m = o.download()
    ids = o.image("ids_after")
    visible = np.zeros(o.count, bool)
    visible[ids[(ids > 0) & (ids < o.count)]] = True
    regime, crafted = craft(orc, m, o.labels(), visible, np.random.default_rng(seed))
    n_crafted = len(regime)
    both_upload(m)                                        # (the frame after the upload carries the fused copy of the segmentation decision's sums)
    regime, crafted, found = find_tagged(o.download()["votes"], regime, crafted)
    print(f"{found} of {n_crafted} crafted surfels in the map after the frame")
    assert found * 10 >= n_crafted * 9
    return g, inst, o, po, masks, cls, regime, crafted, both_upload, lossless


def regime_report(o, regime, crafted, v0, v1, total):
    """From the oracle's downloads and the lossless increments: per regime the surfels whose crafted, voted word changed, and the counters of those words that
    differ from old + increments."""
    n = min(v0.shape[0], v1.shape[0])
    regime, crafted, v0, v1, total = regime[:n], crafted[:n], v0[:n], v1[:n], total[:n]
    voted_w = (total[:, 0::2] + total[:, 1::2]) > 0
    changed_w = crafted & voted_w & (bits(v0) != bits(v1))
    c0, c1 = decode(v0).astype(np.int64), decode(v1).astype(np.int64)
    lossy_c = (c1 != c0 + total) & np.repeat(crafted & voted_w, 2, axis=1)
    ids = o.image("ids_after")
    visible = np.zeros(n, bool)
    visible[ids[(ids > 0) & (ids < n)]] = True
    rep = {}
    for r in NAMES:
        sel = regime == r
        rep[r] = dict(surfels=int(sel.sum()), changed=int(changed_w[sel].any(axis=1).sum()), lossy_counters=int(lossy_c[sel].sum()), visible=int((sel & visible).sum()),
                      hidden=int((sel & ~visible).sum()))
    return rep


def run_calls(ifx, orc, st, n_calls=6):
    g, inst, o, po, masks, cls, regime, crafted, _, lossless = prepare(ifx, orc, st, seed=1, lossless=True)
    rgb, dep = st["rgb"][5], st["depth"][5]
    v0 = o.download()["votes"].copy()
    frame = 200
    if g:
        compare(g, inst, o, "after the upload and a frame", frame, scanned=False)          # (the decision from the frame's fused copy of the sums)
    else:
        o.should_segment(frame)
    for call in range(n_calls):
        frame += 7
        lossless.before()
        if g:
            inst.ProcessSegmentation(rgb, dep, masks, cls, frame)
        o.process_segmentation(rgb, dep, masks, cls, frame)
        lossless.call(rgb, dep, masks, cls, frame)
        if g:
            compare(g, inst, o, f"call {call}", frame + 1)
        else:
            o.should_segment(frame + 1)
    v1 = o.download()["votes"]
    rep = regime_report(o, regime, crafted, v0, v1, lossless.total)
    for r, d in rep.items():
        print(f"{NAMES[r]}: {d}")
    print("instance table:", o.instance_table()[:16].tolist(), " labelled:", int((o.labels() >= 0).sum()))
    lossless.close()
    if g:
        g.close()
    o.close()
    return rep


def check_report(rep):
    for r in (CROSS, TOP, BORROW, RAW):
        assert rep[r]["changed"] >= 100, (NAMES[r], rep[r])
    for r in (CROSS, TOP):
        assert rep[r]["lossy_counters"] >= 100, (NAMES[r], rep[r])
    assert rep[TIE]["visible"] >= 50 and rep[TIE]["hidden"] >= 50, rep[TIE]


def test_calls_in_the_lossy_regimes(ifx, orc, small_stream):
    """Six calls with the frame's canned masks on the crafted map (the first runs the full label scan, the others the per-pixel one), compared after each."""
    t0 = time.perf_counter()
    check_report(run_calls(ifx, orc, small_stream))
    print(f"{time.perf_counter() - t0:.1f} s")


def run_eviction(ifx, orc, st):
    g, inst, o, po, masks, cls, regime, crafted, both_upload, _ = prepare(ifx, orc, st, seed=2)
    rgb, dep = st["rgb"][5], st["depth"][5]
    nm = masks.shape[0]
    evicted, frame = False, 200
    for call in range(40):
        classes = (1000 + call * nm + np.arange(nm)).astype(np.int32)        # a new class for every mask of every call: nothing matches, the table fills
        before = int((o.instance_table() >= 0).sum())
        if before + nm > 96 and not evicted:
            # as test_instance_table_eviction_exact: the calls around the eviction see surfels without a colour yet (colours are assigned once)
            m = o.download(); m["col"][:, 1] = 0.0
            both_upload(m)
        frame += 7
        if g:
            inst.ProcessSegmentation(rgb, dep, masks, classes, frame)
        o.process_segmentation(rgb, dep, masks, classes, frame)
        if g:
            compare(g, inst, o, f"call {call}", frame + 1)
        evicted = evicted or int((o.instance_table() >= 0).sum()) < before
        if evicted and call % 2:
            break
    print(f"{call + 1} calls, table after the eviction: {int((o.instance_table() >= 0).sum())} of 96")
    if g:
        g.close()
    o.close()
    return evicted


def test_eviction_on_the_crafted_map(ifx, orc, small_stream):
    """New classes on every call until the table is full: k_max_count and k_clean_table run on the crafted words; the same outputs after every call."""
    t0 = time.perf_counter()
    assert run_eviction(ifx, orc, small_stream)
    print(f"{time.perf_counter() - t0:.1f} s")
