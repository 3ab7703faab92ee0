"""Seeded adversarial inputs of the superpixel path (SLIC + mergeSuperPixel + the region filter): images on which distance ties, neighbour lists past their cap of
eleven, superpixels that lose every pixel and labels that end without a pixel are the rule and not the exception.  One function per family; image(name, w, h) is a
uint8 (h, w, 3) array, depth(name, w, h) a uint16 (h, w) one (1186 units per metre, as mergeSuperPixel reads it).  Nothing here depends on anything but numpy, and
every array is a function of (name, w, h) alone."""
import numpy as np

IMAGES = ("const", "black", "white", "checker16", "checker8off", "stripes1", "stripes3", "noise", "noise_bin", "centre_dots", "ramp", "blobs")
DEPTHS = ("plane", "tilt", "steps", "noisy", "holes", "zero")

TINY_SIZES = ((64, 48), (72, 56))           # (w, h): every cell a border cell; a partial cell column and row (spn = 15 against 12 centres)
MID_SIZES = ((320, 240), (328, 248))
MID_STORED = ("const", "checker8off", "stripes1", "noise_bin", "blobs")   # the images whose reference labels are stored at MID_SIZES
HANDOVER_SIZES = ((640, 480), (640, 496))   # S = 1200: the last size of the lists-in-LDS connect kernel; S = 1240: the first of the other


def _grid(w, h):
    return np.mgrid[0:h, 0:w]


def _grey(v):
    return np.ascontiguousarray(np.repeat(np.asarray(v, np.uint8)[..., None], 3, -1))


def const(w, h):
    return np.full((h, w, 3), 128, np.uint8)


def black(w, h):
    return np.zeros((h, w, 3), np.uint8)


def white(w, h):
    return np.full((h, w, 3), 255, np.uint8)


def checker16(w, h):
    yy, xx = _grid(w, h)
    return _grey(((xx // 16 + yy // 16) % 2) * 255)


def checker8off(w, h):
    yy, xx = _grid(w, h)
    return _grey((((xx + 8) // 16 + (yy + 8) // 16) % 2) * 255)


def stripes1(w, h):
    yy, xx = _grid(w, h)
    return _grey((xx % 2) * 255)


def stripes3(w, h):
    yy, xx = _grid(w, h)
    return _grey(((yy // 3) % 2) * 255)


def _noise_pair(w, h):
    rng = np.random.RandomState(7)
    a = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    b = (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)   # (from the same generator, after `noise`)
    return a, b


def noise(w, h):
    return _noise_pair(w, h)[0]


def noise_bin(w, h):
    return _noise_pair(w, h)[1]


def centre_dots(w, h):
    img = np.zeros((h, w, 3), np.uint8)
    img[8::16, 8::16] = 255     # the initial centres of SLIC, and nothing else
    return img


def ramp(w, h):
    yy, xx = _grid(w, h)
    return np.ascontiguousarray(np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), (xx + yy) % 256], -1).astype(np.uint8))


def blobs(w, h):
    rng = np.random.RandomState(12)
    yy, xx = _grid(w, h)
    img = np.zeros((h, w, 3), np.uint8)
    for _ in range(12):
        cx, cy, r = rng.randint(0, w), rng.randint(0, h), rng.randint(3, 30)
        col = rng.randint(0, 256, 3)
        img[(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = col
    return img


def image(name, w, h):
    assert name in IMAGES, name
    return globals()[name](w, h)


def plane(w, h):
    return np.full((h, w), 2372, np.uint16)     # 2 m


def tilt(w, h):
    yy, xx = _grid(w, h)
    return (1500 + 4 * xx + 2 * yy).astype(np.uint16)


def steps(w, h):
    yy, xx = _grid(w, h)
    return (1200 + 600 * ((xx // 40 + yy // 40) % 3)).astype(np.uint16)


def noisy(w, h):
    return (2000 + np.random.RandomState(21).randint(-60, 61, (h, w))).astype(np.uint16)


def holes(w, h):
    d = tilt(w, h)
    d[np.random.RandomState(22).rand(h, w) < 0.05] = 0
    return d


def zero(w, h):
    return np.zeros((h, w), np.uint16)


def depth(name, w, h):
    assert name in DEPTHS, name
    return globals()[name](w, h)


def camera(w, h):
    """The intrinsics every test of this family gives its handles (the 640-wide camera of the other superpixel tests, scaled)."""
    return dict(fx=528.0 * w / 640, fy=528.0 * w / 640, cx=w / 2.0, cy=h / 2.0)


def golden_cases():
    """(image, w, h) of every array in tests/golden/slic_cases_ref.npz, stored under key(...)."""
    out = [(n, w, h) for (w, h) in TINY_SIZES for n in IMAGES]
    out += [(n, w, h) for (w, h) in MID_SIZES for n in MID_STORED]
    return out


def key(name, w, h):
    return f"{name}_{w}x{h}"


def sprinkle(seg, spn):
    """(seg with the ids -5, spn and 10**6 sprinkled in, the same labelling with -1 at those pixels)."""
    a, b = seg.copy(), seg.copy()
    for val, (ys, xs) in ((-5, (slice(0, None, 7), slice(0, None, 5))), (spn, (slice(3, None, 11), slice(2, None, 9))), (10 ** 6, (slice(5, None, 13), slice(1, None, 6)))):
        a[ys, xs] = val
        b[ys, xs] = -1
    return a, b


def neighbour_counts(seg, spn):
    """Distinct 4-neighbour labels of every label, over the interior pixels -- the relation k_sp_sums / kernel B collects before the cap of eleven."""
    s = seg.astype(np.int64)
    pairs = []
    a = s[1:-1, 1:-1]
    for b in (s[2:, 1:-1], s[:-2, 1:-1], s[1:-1, 2:], s[1:-1, :-2]):
        m = (a >= 0) & (b >= 0) & (a != b)
        pairs.append(a[m] * spn + b[m])
    u = np.unique(np.concatenate(pairs)) if pairs else np.zeros(0, np.int64)
    return np.bincount(u // spn, minlength=spn)
