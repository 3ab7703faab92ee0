"""Seeded adversarial inputs of the geometric mask filter (maskGeometricFilter: the flood fill along source-threshold edges, the 25 % rule per region, the 65 %
rule per mask): one-pixel corridors that cross every tile border of the device's 32 x 32 tiling, regions that hang together through one pixel pair on a tile border,
depth steps that meet the threshold exactly, region sizes that meet the two ratios exactly, masks on the image border, 256 masks.  Every builder returns
(w, h, depth u16 (h, w), masks u8 (n, h, w), ori u8 (n, h, w), unavailable u8 (n,)); nothing here depends on anything but numpy and every array is a function of
the builder's arguments alone.  The depth is the MODEL depth the filter reads: 1186 units per metre, 0 = no surfel under the pixel."""
import numpy as np

SIZES = ((36, 36), (68, 44))        # (w, h): one tile plus a ragged 4; ragged both ways with tile borders inside the image in both directions
BIG = (320, 240)
SAW = (5000, 4880, 4910, 4940, 4970)    # along the serpentine: the drop of 120 is an edge from 5000 only (threshold 124 there, 115.12 at 4880); the steps of 30 are two-way


def threshold(depth):
    """getDepthThreshold in float32, for an integer array."""
    t = np.float32(0.074) * np.asarray(depth).astype(np.float32) - np.float32(246.0)
    return np.minimum(np.float32(420.0), np.maximum(np.float32(50.0), t)).astype(np.float32)


def fill_pixels(depth, mask):
    """The pixels the fill visits: interior, mask set, model depth valid."""
    v = (np.asarray(mask) != 0) & (np.asarray(depth) != 0)
    v[0, :] = v[-1, :] = False
    v[:, 0] = v[:, -1] = False
    return v


def one_way_edges(depth, mask):
    """Pairs of 4-neighbours, both visited by the fill of `mask`, joined by an edge in exactly one direction."""
    d = np.asarray(depth).astype(np.int32)
    v, t = fill_pixels(depth, mask), threshold(depth)
    n = 0
    for a, b in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:-1, :], np.s_[1:, :])):
        dd = np.abs(d[a] - d[b]).astype(np.float32)
        n += int((v[a] & v[b] & ((dd < t[a]) != (dd < t[b]))).sum())
    return n


def _pack(w, h, depth, masks, ori=None, un=None):
    masks = np.ascontiguousarray(masks, np.uint8)
    ori = masks.copy() if ori is None else np.ascontiguousarray(ori, np.uint8)
    un = np.zeros(masks.shape[0], np.uint8) if un is None else np.ascontiguousarray(un, np.uint8)
    assert depth.shape == (h, w) and depth.dtype == np.uint16 and masks.shape == ori.shape == (un.shape[0], h, w) and w >= 32 and h >= 32
    return w, h, depth, masks, ori, un


# ---------------------------------------------------------------- serpentine
def serpentine_path(w, h, last_row=None):
    """(ys, xs) along a one-pixel corridor: rows 1, 3, 5, ... (up to last_row, by default h - 2), joined alternately at the right and the left end."""
    ys, xs = [], []
    y, d = 1, 1
    h = h if last_row is None else last_row + 2
    while y <= h - 2:
        row = range(1, w - 1) if d > 0 else range(w - 2, 0, -1)
        for x in row:
            ys.append(y); xs.append(x)
        if y + 2 > h - 2:
            break
        ys.append(y + 1); xs.append(xs[-1])
        y += 2; d = -d
    return np.asarray(ys), np.asarray(xs)


def serpentine(w, h, reverse=False, last_row=None):
    """The corridor with SAW repeated along it.  Forward: the path starts at the first pixel in row-major order, which therefore reaches every pixel -- one region,
    found only by carrying one label along the whole path (through every tile, back and forth).  reverse: the same corridor walked from its other end (bottom right),
    the mirror image: every pixel is reached by all pixels BEHIND it on the path, so rows walked left to right are one region each (their first pixel), rows
    walked right to left fall into the two-way groups of five -- labels flow in both directions in alternate rows.  There `ori` is the first two rows of the corridor
    only (except at 320 x 240, where more than 20 rows would qualify and `ori` stays the mask: nothing is kept): a quarter of it is half a row, the whole-row
    regions are kept, the groups of five are not.  last_row: the corridor ends there (rows below stay free for another mask)."""
    ys, xs = serpentine_path(w, h, last_row)
    seq = np.asarray(SAW, np.uint16)[np.arange(len(ys)) % 5]
    depth = np.zeros((h, w), np.uint16)
    depth[ys, xs] = seq[::-1] if reverse else seq
    masks = np.zeros((1, h, w), np.uint8)
    masks[0, ys, xs] = 255
    ori = masks.copy()
    if reverse and (w, h) != BIG:
        ori[0, 4:] = 0
    return _pack(w, h, depth, masks, ori)


# ---------------------------------------------------------------- regions that exist only through tile-border edges
def _blob_pair(depth, mask, horizontal, first_depth, second_depth, second_earlier):
    """A small blob (45 pixels with its bridge pixel) and a large one (144) in neighbouring tiles, joined by ONE pixel pair across the border 31 | 32.  As two regions
    the small one is 23.8 % of the mask and is dropped.  Vertical border: small blob left, large right; second_earlier starts the large blob two rows higher, so
    that it holds the first pixel in row-major order.  Horizontal border: small blob above, always the earlier one."""
    yy, xx = np.mgrid[0:depth.shape[0], 0:depth.shape[1]]
    if not horizontal:
        top = 3 if second_earlier else 5
        a = (xx >= 20) & (xx <= 30) & (yy >= 5) & (yy <= 8)
        b = (xx >= 33) & (xx <= 45) & (yy >= top) & (yy <= top + 10)
        a[7, 31] = True; b[7, 32] = True
    else:
        a = (yy >= 27) & (yy <= 30) & (xx >= 5) & (xx <= 15)
        b = (yy >= 33) & (yy <= 40) & (xx >= 3) & (xx <= 20)
        a[31, 9] = True; b[32, 9] = True
    depth[a] = first_depth; depth[b] = second_depth
    mask[a | b] = 255


TILE_BORDER = (   # name, horizontal border, depth of the first blob, of the second, second blob earlier, one region
    ("v_two_way", False, 2000, 2010, False, True), ("h_two_way", True, 2000, 2010, False, True),
    ("v_left_to_right_left_earlier", False, 5000, 4880, False, True), ("v_right_to_left_left_earlier", False, 4880, 5000, False, False),
    ("v_left_to_right_right_earlier", False, 5000, 4880, True, False), ("v_right_to_left_right_earlier", False, 4880, 5000, True, True),
    ("h_top_to_bottom", True, 5000, 4880, False, True), ("h_bottom_to_top", True, 4880, 5000, False, False),
    ("diagonal", None, 2000, 2000, False, False),
)


def tile_border():
    """68 x 44, one case (one mask, a depth image of its own) per row of TILE_BORDER: the list of (name, one_region, case)."""
    w, h = 68, 44
    out = []
    for name, horizontal, d1, d2, second_earlier, one in TILE_BORDER:
        depth = np.full((h, w), 3000, np.uint16)
        masks = np.zeros((1, h, w), np.uint8)
        ori = None
        if horizontal is None:      # two blocks of 49 that touch at the tile corner only: 22.5 % each of an `ori` of 218 -- dropped apart, kept as one
            masks[0, 25:32, 25:32] = 255; masks[0, 32:39, 32:39] = 255
            ori = masks.copy(); ori[0, 2:12, 2:14] = 255
            assert int((ori[0] != 0).sum()) == 218
        else:
            _blob_pair(depth, masks[0], horizontal, d1, d2, second_earlier)
        out.append((name, one, _pack(w, h, depth, masks, ori)))
    return out


# ---------------------------------------------------------------- thresholds met exactly
# (source depth a, neighbour depth b, edge a -> b, edge b -> a): threshold(a) is 50 below 4000, 0.074 a - 246 above, 420 from 9000
STEPS = (
    (3000, 3049, 1, 1), (3000, 3050, 0, 0), (3000, 3051, 0, 0), (3000, 2951, 1, 1), (3000, 2950, 0, 0),
    (9500, 9919, 1, 1), (9500, 9920, 0, 0), (9500, 9921, 0, 0), (9500, 9081, 1, 1), (9500, 9080, 0, 0),
    (5000, 4877, 1, 0), (5000, 4876, 0, 0), (5000, 4875, 0, 0), (5000, 5123, 1, 1), (5000, 5124, 0, 1), (5000, 5125, 0, 1),
    (4100, 4045, 1, 0), (4000, 4060, 0, 0),
    (65535, 65200, 1, 1), (65535, 65116, 1, 1), (65535, 65115, 0, 0), (65535, 0, 0, 0),
)


def steps(vertical=False):
    """68 x 44.  Every entry of STEPS as strips of 10 pixels, 8 at a first depth and 2 at a second: the strip is one region iff the edge first -> second exists
    (the first pixel is the earlier one); apart, the 2 are 20 % of the mask and are dropped.  Four masks per entry: a first or b first, each with the junction inside
    a tile and on a tile border (31 | 32, for b first in rows 63 | 64).  vertical: the strips run down the columns, the junction on the horizontal border 31 | 32.
    Returns (case, expect): expect[m] = pixels kept of mask m -- 10 or 8; where a depth is 0 the valid pixels are the others: 8 of 10 kept, 2 of 10 dropped."""
    w, h = 68, 44
    depth = np.zeros((h, w), np.uint16)
    masks, expect = [], []
    for i, (a, b, ab, ba) in enumerate(STEPS):
        for order, (first, second, joined) in enumerate(((a, b, ab), (b, a, ba))):
            for on_border in (0, 1):
                m = np.zeros((h, w), np.uint8)
                if vertical:
                    line, s0 = 1 + 2 * i + order, (24 if on_border else 2)
                    depth[s0:s0 + 8, line] = first; depth[s0 + 8:s0 + 10, line] = second
                    m[s0:s0 + 10, line] = 255
                else:
                    line, s0 = 1 + i, ((2, 24), (36, 56))[order][on_border]
                    depth[line, s0:s0 + 8] = first; depth[line, s0 + 8:s0 + 10] = second
                    m[line, s0:s0 + 10] = 255
                masks.append(m)
                expect.append(0 if first == 0 else 8 if second == 0 or not joined else 10)
    return _pack(w, h, depth, np.stack(masks)), np.asarray(expect)


# ---------------------------------------------------------------- ratios met exactly (near depth: every edge two-way, regions = blocks)
RATIOS = ("quarter_100_of_400", "quarter_101_of_400", "four_quarters", "three_of_30", "total_65", "total_64", "ori_empty", "both_empty", "ori_on_border_only",
          "ori_empty_24_regions", "ori_small_24_regions")
# what the reference's float32 arithmetic gives: (pixels kept, unavailable afterwards)
RATIO_EXPECT = dict(quarter_100_of_400=(0, 1), quarter_101_of_400=(101, 1), four_quarters=(0, 1), three_of_30=(90, 0), total_65=(65, 0), total_64=(64, 1),
                    ori_empty=(30, 0), both_empty=(0, 0), ori_on_border_only=(30, 0), ori_empty_24_regions=(80, 0), ori_small_24_regions=(40, 0))


def ratios(w, h):
    """One mask per name in RATIOS.  points / oriPoints > 0.25 keeps a region, finalPoints / oriPoints < 0.65 makes the mask unusable; with oriPoints = 0 the
    first is inf (kept) or never evaluated, the second inf or NaN (usable either way).  The last two hold 24 regions that all qualify -- possible only where `ori`
    is far smaller than the mask: the reference's list takes the FIRST twenty in scan order."""
    depth = np.full((h, w), 2000, np.uint16)
    n = len(RATIOS)
    masks, ori = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.uint8)

    def block(a, i, y, x, count, width=10):     # `count` pixels from (y, x), rows of `width`
        for k in range(count):
            a[i, y + k // width, x + k % width] = 255

    i = RATIOS.index("quarter_100_of_400")
    ori[i, 2:22, 2:22] = 255; block(masks, i, 2, 2, 100)
    i = RATIOS.index("quarter_101_of_400")
    ori[i, 2:22, 2:22] = 255; block(masks, i, 2, 2, 101, width=5)    # (21 rows: reaches row 22, outside `ori` -- the mask need not lie inside it)
    block(masks, i, 2, 10, 100)                                       # and a second region of exactly 100 next to it, not kept
    i = RATIOS.index("four_quarters")
    for k in range(4):
        block(masks, i, 2 + 8 * (k // 2), 2 + 8 * (k % 2), 25, width=5)
    ori[i] = masks[i]
    i = RATIOS.index("three_of_30")
    for k in range(3):
        block(masks, i, 2 + 5 * k, 2, 30)
    ori[i] = masks[i]; block(ori, i, 20, 2, 10)
    i = RATIOS.index("total_65")
    block(ori, i, 2, 2, 100); block(masks, i, 2, 2, 65)
    i = RATIOS.index("total_64")
    block(ori, i, 2, 2, 100); block(masks, i, 2, 2, 64)
    i = RATIOS.index("ori_empty")
    block(masks, i, 5, 5, 30)
    i = RATIOS.index("ori_on_border_only")
    block(masks, i, 5, 5, 30); ori[i, 0, :] = 255; ori[i, :, w - 1] = 255
    for k in range(24):     # a 6 x 4 grid of separate blocks, rows 2, 10, 18, 26: the last four blocks do not fit into the list
        y, x = 2 + 8 * (k // 6), 2 + 5 * (k % 6)
        masks[RATIOS.index("ori_empty_24_regions"), y:y + 2, x:x + 2] = 255
        masks[RATIOS.index("ori_small_24_regions"), y, x:x + 2] = 255
    ori[RATIOS.index("ori_small_24_regions"), 30, 2:6] = 255
    return _pack(w, h, depth, masks, ori)


# ---------------------------------------------------------------- borders, checkerboard, zero depth, everything unavailable
def borders(w, h):
    """Masks on the outermost rows and columns (never interior, always cleared), the whole frame (a region from x = 1 to x = w - 2) and a frame-shaped ring."""
    depth = np.full((h, w), 2500, np.uint16)
    masks = np.zeros((4, h, w), np.uint8)
    masks[0, 0, :] = masks[0, -1, :] = 255; masks[0, :, 0] = masks[0, :, -1] = 255
    masks[1] = 255
    masks[2, :3, :] = masks[2, -3:, :] = 255; masks[2, :, :3] = masks[2, :, -3:] = 255
    masks[3, h // 2, :] = 255       # one row from edge to edge
    return _pack(w, h, depth, masks)


def checkerboard(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    masks = np.stack([((xx + yy) % 2 == 0) * 255, ((xx + yy) % 2 == 1) * 255]).astype(np.uint8)
    return _pack(w, h, np.full((h, w), 2500, np.uint16), masks)


def zero_depth(w, h):
    masks = np.zeros((2, h, w), np.uint8)
    masks[0, 4:20, 4:30] = 255; masks[1] = 255
    return _pack(w, h, np.zeros((h, w), np.uint16), masks)


def all_unavailable(w, h):
    w, h, depth, masks, ori, un = random_case(w, h, 0)
    return _pack(w, h, depth, masks, ori, np.ones_like(un))


# ---------------------------------------------------------------- random family
def far_depth(w, h, rng, amplitude=1.0):
    """A ramp from 3000 to 11000 along the diagonal (73 units a pixel at 68 x 44, 114 at 36 x 36: more than the threshold of 50 at its near end, less further out)
    plus noise whose amplitude is `amplitude` times the local threshold, with 2 % holes."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 3000 + 8000 * (xx + yy) / (w + h - 2)
    noise = (rng.rand(h, w) * 2 - 1) * amplitude * threshold(base.astype(np.int32))
    d = np.clip(base + noise, 1, 65535).astype(np.uint16)
    d[rng.rand(h, w) < 0.02] = 0
    return d


def random_case(w, h, seed, n=8):
    """n masks, unions of random rectangles and discs; `ori` the mask dilated by 0 to 3 pixels; noise amplitude between 0.3 and 1.1 of the local threshold."""
    rng = np.random.RandomState(1000 * w + seed)
    depth = far_depth(w, h, rng, (0.3, 0.5, 0.7, 0.8, 0.95, 1.1)[seed % 6])
    yy, xx = np.mgrid[0:h, 0:w]
    masks, ori = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.uint8)
    for i in range(n):
        m = np.zeros((h, w), bool)
        for _ in range(rng.randint(1, 4)):
            if rng.rand() < 0.5:
                x0, y0 = rng.randint(0, w - 6), rng.randint(0, h - 6)
                m[y0:y0 + rng.randint(4, h // 2), x0:x0 + rng.randint(4, w // 2)] = True
            else:
                cx, cy, r = rng.randint(0, w), rng.randint(0, h), rng.randint(3, min(w, h) // 3)
                m |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
        o = m.copy()
        for _ in range(rng.randint(0, 4)):      # dilation by one pixel, 4-neighbourhood, 0 to 3 times
            g = o.copy()
            g[1:] |= o[:-1]; g[:-1] |= o[1:]; g[:, 1:] |= o[:, :-1]; g[:, :-1] |= o[:, 1:]
            o = g
        masks[i][m] = 255; ori[i][o] = 255
    return _pack(w, h, depth, masks, ori)


RANDOM_SEEDS = tuple(range(6))


# ---------------------------------------------------------------- 256 masks, the documented limit
def many_masks(n=256, seed=0):
    """68 x 44: mask m is a rectangle of its own size in cell m of a 16 x 16 grid of 4 x 2 cells (cells repeat beyond 256 masks: n = 257 is only ever refused),
    grown by a few pixels into its neighbours for every third mask so that regions differ; `ori` = mask, for every fifth mask the whole 4 x 2 cell block around
    it; every eighth mask is unavailable on entry."""
    w, h = 68, 44
    rng = np.random.RandomState(77 + seed)
    depth = far_depth(w, h, rng, 0.6)
    masks, ori = np.zeros((n, h, w), np.uint8), np.zeros((n, h, w), np.uint8)
    for m in range(n):
        c = m % 256
        x0, y0 = 2 + 4 * (c % 16), 2 + 2 * (c // 16)
        ww, hh = 1 + c % 4, 1 + (c // 4) % 2
        if m % 3 == 0:
            ww += 5; hh += 3
        masks[m, y0:y0 + hh, x0:x0 + ww] = 255
        ori[m] = masks[m]
        if m % 5 == 0:
            ori[m, max(y0 - 2, 0):y0 + hh + 2, max(x0 - 3, 0):x0 + ww + 3] = 255
    un = (np.arange(n) % 8 == 7).astype(np.uint8)
    return _pack(w, h, depth, masks, ori, un)


def sequence():
    """Calls on ONE handle at 68 x 44 with n = 3, 256, 1, 40: the fill's scratch grows, then is reused with fewer masks (stale labels and counters behind them)."""
    out = []
    for n, seed in ((3, 1), (256, 2), (1, 3), (40, 4)):
        if n in (3, 1):
            w, h, depth, masks, ori, un = random_case(68, 44, 10 + seed, n=n)
        else:
            w, h, depth, masks, ori, un = many_masks(n, seed)
        out.append(_pack(w, h, depth, masks, ori, un))
    return out


def small_cases():
    """name -> case, every case up to 68 x 44 (the sequence's steps and the tile-border list included)."""
    out = {}
    for (w, h) in SIZES:
        s = f"{w}x{h}"
        out[f"serpentine_{s}"] = serpentine(w, h)
        out[f"serpentine_reverse_{s}"] = serpentine(w, h, reverse=True)
        out[f"ratios_{s}"] = ratios(w, h)
        out[f"borders_{s}"] = borders(w, h)
        out[f"checkerboard_{s}"] = checkerboard(w, h)
        out[f"zero_depth_{s}"] = zero_depth(w, h)
        out[f"all_unavailable_{s}"] = all_unavailable(w, h)
        for seed in RANDOM_SEEDS:
            out[f"random_{s}_{seed}"] = random_case(w, h, seed)
    for name, _, case in tile_border():
        out[f"tile_border_{name}"] = case
    out["steps_rows"] = steps(False)[0]
    out["steps_columns"] = steps(True)[0]
    out["many_masks_256"] = many_masks()
    for k, case in enumerate(sequence()):
        out[f"sequence_{k}"] = case
    return out


def big_cases():
    return {"serpentine_320x240": serpentine(*BIG), "serpentine_reverse_320x240": serpentine(*BIG, reverse=True)}
