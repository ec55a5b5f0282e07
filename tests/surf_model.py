"""NumPy restatement of svs_surf_extract (include/scavislam_hip.h, "loop closure, the start of PlaceRecognizer::addLocation", points 1-8): the yardstick of
tests/test_surf_cpu.py and tests/test_gpu_surf.py.  Whole-image operations and plain loops, no tiling, nothing of the kernels' structure.  f32 arithmetic is
NumPy float32 arithmetic (every operation rounds once), sequential f32 sums are np.cumsum (sequential), the transcendental functions are libm's through `math`.

extract() also reports, per keypoint, the BANDS in which a last-bit difference of a transcendental function could change a discrete decision.  Both sides form
every angle, sine and cosine as the f64 function rounded to f32, so two faithful implementations differ by at most one f32 ulp there, and the bands are exactly
as wide as that (blanket widths of 1e-3 degrees / 1e-4 px would hold most keypoints: a window has up to 2 x 151^2 coordinates):
  a sample angle within 1e-4 degrees (3 ulp at 360) of a cvRound tie; the two best (distinct) windows within 1e-5 relative; a window whose sampled pixels change
  when sin_dir / cos_dir move by one ulp either way (all eight neighbours are tried).  The patch follows from the sampled pixels without another transcendental."""
import math

import numpy as np

F = np.float32
DEG = 57.29577951308232
DX = [(0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1)]
DY = [(2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1)]
DXY = [(1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1)]
DXS = [(0, 0, 2, 4, -1), (2, 0, 4, 4, 1)]
DYS = [(0, 0, 4, 2, 1), (0, 2, 4, 4, -1)]
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("laplacian", "<i4"), ("pad_", "<i4")])
assert KP_DTYPE.itemsize == 32


def cvround(v):
    return int(np.rint(np.float64(v)))


def c_round(v):
    v = float(v)
    return math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)


def gaussian(n, sigma):
    scale2 = -0.5 / (sigma * sigma)
    cf = [F(math.exp(scale2 * (i - (n - 1) * 0.5) * (i - (n - 1) * 0.5))) for i in range(n)]
    s = 0.0
    for c in cf:
        s += float(c)
    s = 1.0 / s
    return np.array([F(float(c) * s) for c in cf], F)


G_ORI, G_DESC = gaussian(13, 2.5), gaussian(20, 3.3)
ORI = [(i, j, G_ORI[i + 6] * G_ORI[j + 6]) for i in range(-6, 7) for j in range(-6, 7) if i * i + j * j <= 36]
assert len(ORI) == 113
DW = np.outer(G_DESC, G_DESC).astype(F)      # f32 x f32 products


def integral(img):
    h, w = img.shape
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.int64), 0), 1)
    assert S.max() < 2 ** 31
    return S


def scale_pattern(src, old, new):
    ratio = F(new) / F(old)
    out = []
    for (x1, y1, x2, y2, wt) in src:
        a, b, c, d = (cvround(ratio * F(v)) for v in (x1, y1, x2, y2))
        out.append((a, b, c, d, F(wt) / (F(c - a) * F(d - b))))
    return out


def haar(S, ys, xs, boxes):
    """pattern value at the origins ys x xs: a double accumulator of f32 products, cast to float"""
    acc = np.zeros((len(ys), len(xs)), np.float64)
    for (x1, y1, x2, y2, wt) in boxes:
        v = S[np.ix_(ys + y1, xs + x1)] + S[np.ix_(ys + y2, xs + x2)] - S[np.ix_(ys + y2, xs + x1)] - S[np.ix_(ys + y1, xs + x2)]
        acc += (v.astype(F) * wt).astype(np.float64)
    return acc.astype(F)


def layers(S, n_octaves=2, n_layers=2):
    """[(octave, layer, size, step, det, trace)]"""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    out = []
    for o in range(n_octaves):
        for l in range(n_layers + 2):
            size, step = (9 + 6 * l) << o, 1 << o
            det, tr = np.zeros((h // step, w // step), F), np.zeros((h // step, w // step), F)
            si, sj, m = 1 + (h - size) // step, 1 + (w - size) // step, (size // 2) // step
            if h >= size and w >= size:
                ys, xs = np.arange(si) * step, np.arange(sj) * step
                dx, dy, dxy = (haar(S, ys, xs, scale_pattern(p, 9, size)) for p in (DX, DY, DXY))
                det[m:m + si, m:m + sj] = dx * dy - (F(0.81) * dxy) * dxy
                tr[m:m + si, m:m + sj] = dx + dy
            out.append((o, l, size, step, det, tr))
    return out


def lu_solve3(A, b):
    """the header's LU; None: no solution"""
    A = [[F(v) for v in r] for r in A]
    b = [F(v) for v in b]
    for r in range(3):
        k = r
        for q in range(r + 1, 3):
            if abs(A[q][r]) > abs(A[k][r]):
                k = q
        if not abs(A[k][r]) >= F(np.finfo(F).eps) * F(10):
            return None
        if k != r:
            A[r], A[k] = A[k], A[r]
            b[r], b[k] = b[k], b[r]
        d = F(-1) / A[r][r]
        for q in range(r + 1, 3):
            alpha = A[q][r] * d
            for s in range(r + 1, 3):
                A[q][s] = A[q][s] + alpha * A[r][s]
            b[q] = b[q] + alpha * b[r]
        A[r][r] = -d
    for r in (2, 1, 0):
        s = b[r]
        for q in range(r + 1, 3):
            s = s - A[r][q] * b[q]
        b[r] = s * A[r][r]
    return b


def maxima(lay, threshold, n_layers=2):
    """refined maxima as dicts, in no particular order"""
    out = []
    per = n_layers + 2
    with np.errstate(all="ignore"):
        for k, (o, l, size, step, det, tr) in enumerate(lay):
            if l < 1 or l > n_layers:
                continue
            lo, hi = lay[k - 1], lay[k + 1]
            rows, cols = det.shape
            border = (hi[2] // 2) // step + 1
            if rows - 2 * border <= 0 or cols - 2 * border <= 0:
                continue
            c = det[border:rows - border, border:cols - border]
            ok = c > F(threshold)
            for q, L in enumerate((lo[4], det, hi[4])):
                for r in (-1, 0, 1):
                    for s in (-1, 0, 1):
                        if q == 1 and r == 0 and s == 0:
                            continue
                        ok &= c > L[border + r:rows - border + r, border + s:cols - border + s]
            for (ii, jj) in zip(*np.nonzero(ok)):
                i, j = int(ii) + border, int(jj) + border
                N = [[L[i + r - 1, j + s - 1] for r in range(3) for s in range(3)] for L in (lo[4], det, hi[4])]
                half = F(size - 1) * F(0.5)
                cy, cx = F(step * (i - (size // 2) // step)) + half, F(step * (j - (size // 2) // step)) + half
                two, four = F(2), F(4)
                b = [-(N[1][5] - N[1][3]) / two, -(N[1][7] - N[1][1]) / two, -(N[2][4] - N[0][4]) / two]
                dxy = (N[1][8] - N[1][6] - N[1][2] + N[1][0]) / four
                dxs = (N[2][5] - N[2][3] - N[0][5] + N[0][3]) / four
                dys = (N[2][7] - N[2][1] - N[0][7] + N[0][1]) / four
                A = [[N[1][3] - two * N[1][4] + N[1][5], dxy, dxs], [dxy, N[1][1] - two * N[1][4] + N[1][7], dys], [dxs, dys, N[0][4] - two * N[1][4] + N[2][4]]]
                x = lu_solve3(A, b)
                if x is None or not ((x[0] != 0 or x[1] != 0 or x[2] != 0) and all(abs(v) <= 1 for v in x)):
                    continue
                t = tr[i, j]
                out.append(dict(x=cx + x[0] * F(step), y=cy + x[1] * F(step), size=F(cvround(F(size) + x[2] * F(size - lo[2]))), response=det[i, j], octave=o,
                                laplacian=int(t > 0) - int(t < 0), layer=l, ij=i * cols + j))
    return out


def order_key(c):
    return (-float(c["response"]), -float(c["size"]), float(c["y"]), float(c["x"]), c["octave"], c["layer"], c["ij"])


def disparity_rule(disp, x, y):
    """None: dropped; else uvu (f64)"""
    h, w = disp.shape
    rx, ry = c_round(x), c_round(y)
    if not (0 <= rx < w and 0 <= ry < h):
        return None
    d = float(disp[int(ry), int(rx)])
    if not d > 0:
        return None
    u2 = float(x) - d
    if not float(x) - u2 > 0:      # d below half an ulp of x
        return None
    return np.array([float(x), float(y), u2], np.float64)


def degrees(y, x):
    a = math.atan2(float(y), float(x)) * DEG
    if a < 0:
        a = a + 360.0
    return F(a)


def box_value(S, y, x, boxes):
    d = 0.0
    for (x1, y1, x2, y2, wt) in boxes:
        v = int(S[y + y1, x + x1] + S[y + y2, x + x2] - S[y + y2, x + x1] - S[y + y1, x + x2])
        d += float(F(v) * wt)
    return F(d)


def orientation(S, kp):
    """None: removed; else (angle, dir, alt_angle, band)"""
    h, w = S.shape[0] - 1, S.shape[1] - 1
    s = kp["size"] * F(1.2) / F(9.0)
    gws = 2 * cvround(F(2) * s)
    if h + 1 < gws or w + 1 < gws:
        return None
    bx, by = scale_pattern(DXS, 4, gws), scale_pattern(DYS, 4, gws)
    off = F(gws - 1) / F(2)
    X, Y, A = [], [], []
    band = False
    for (i, j, wt) in ORI:
        x, y = cvround((kp["x"] + F(i) * s) - off), cvround((kp["y"] + F(j) * s) - off)
        if y < 0 or y >= h + 1 - gws or x < 0 or x >= w + 1 - gws:
            continue
        vx, vy = box_value(S, y, x, bx) * wt, box_value(S, y, x, by) * wt
        a = degrees(vy, vx)
        band |= abs(float(a) - math.floor(float(a)) - 0.5) < 1e-4
        X.append(vx), Y.append(vy), A.append(cvround(a))
    if not X:
        return None
    X, Y, A = np.array(X, F), np.array(Y, F), np.array(A)
    wins = []
    for q in range(72):
        d = np.abs(A - 5 * q)
        m = (d < 30) | (d > 330)
        sx = np.cumsum(X[m], dtype=F)[-1] if m.any() else F(0)
        sy = np.cumsum(Y[m], dtype=F)[-1] if m.any() else F(0)
        wins.append((sx * sx + sy * sy, sx, sy))
    best = (F(0), F(0), F(0))
    for wn in wins:
        if wn[0] > best[0]:
            best = wn
    second = None
    for wn in wins:
        if (wn[1], wn[2]) != (best[1], best[2]) and (second is None or wn[0] > second[0]):
            second = wn

    def angle_of(wn):
        d = degrees(wn[2], wn[1])
        a = F(360) - d
        return (F(0) if abs(a - F(360)) < np.finfo(F).eps else a), d
    ang, d = angle_of(best)
    alt = ang
    if second is not None and float(best[0]) > 0 and float(best[0] - second[0]) <= 1e-5 * float(best[0]):
        band = True
        alt = angle_of(second)[0]
    return ang, d, alt, band


def area_tab(ssize, dsize=21):
    scale = ssize / dsize
    tab = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            tab.append((d, s1 - 1, F((s1 - f1) / cell)))
        for sx in range(s1, s2):
            tab.append((d, sx, F(1.0 / cell)))
        if f2 - s2 > 1e-3:
            tab.append((d, s2, F(min(min(f2 - s2, 1.0), cell) / cell)))
    return tab


def window_pixels(img, kp, win, sin_dir, cos_dir):
    """the win x win source coordinates (running f32 sums, cvRound, clamped)"""
    h, w = img.shape
    off = -F(win - 1) / F(2)
    a, b = off * cos_dir, off * sin_dir
    sx0, sy0 = (kp["x"] + a) + b, (kp["y"] - b) + a
    start_x = np.cumsum(np.concatenate([[sx0], np.full(win - 1, sin_dir, F)]).astype(F), dtype=F)
    start_y = np.cumsum(np.concatenate([[sy0], np.full(win - 1, cos_dir, F)]).astype(F), dtype=F)
    px = np.cumsum(np.concatenate([start_x[:, None], np.full((win, win - 1), cos_dir, F)], 1).astype(F), axis=1, dtype=F)
    py = np.cumsum(np.concatenate([start_y[:, None], np.full((win, win - 1), -sin_dir, F)], 1).astype(F), axis=1, dtype=F)
    xi = np.clip(np.rint(px.astype(np.float64)).astype(np.int64), 0, w - 1)
    yi = np.clip(np.rint(py.astype(np.float64)).astype(np.int64), 0, h - 1)
    return yi, xi


def descriptor(img, kp, dir_deg, with_band=True):
    """(64 floats, band)"""
    s = kp["size"] * F(1.2) / F(9.0)
    win = int(F(21) * s)
    rad = F(dir_deg) * F(math.pi / 180)
    sin_dir, cos_dir = F(math.sin(float(rad))), F(math.cos(float(rad)))
    yi, xi = window_pixels(img, kp, win, sin_dir, cos_dir)
    WIN = img[yi, xi].astype(F)
    band = False
    if with_band:
        for ds in (-1, 0, 1):
            for dc in (-1, 0, 1):
                if (ds or dc) and not band:
                    s2 = np.nextafter(sin_dir, F(np.inf * ds)) if ds else sin_dir
                    c2 = np.nextafter(cos_dir, F(np.inf * dc)) if dc else cos_dir
                    y2, x2 = window_pixels(img, kp, win, s2, c2)
                    band = not np.array_equal(img[y2, x2], img[yi, xi])
    tab = area_tab(win)
    buf = np.zeros((win, 21), F)
    for (d, si, al) in tab:
        buf[:, d] = buf[:, d] + WIN[:, si] * al
    acc = np.zeros((21, 21), F)
    for (d, si, be) in tab:
        acc[d, :] = acc[d, :] + be * buf[si, :]
    P = np.clip(np.rint(acc.astype(np.float64)), 0, 255).astype(np.int64)
    vx = (P[:20, 1:] - P[:20, :20] + P[1:, 1:] - P[1:, :20]).astype(F) * DW
    vy = (P[1:, :20] - P[:20, :20] + P[1:, 1:] - P[:20, 1:]).astype(F) * DW
    vec = np.zeros(64, F)
    for ci in range(4):
        for cj in range(4):
            tx, ty = vx[5 * ci:5 * ci + 5, 5 * cj:5 * cj + 5].reshape(-1), vy[5 * ci:5 * ci + 5, 5 * cj:5 * cj + 5].reshape(-1)
            k = 4 * (4 * ci + cj)
            vec[k], vec[k + 1] = np.cumsum(tx, dtype=F)[-1], np.cumsum(ty, dtype=F)[-1]
            vec[k + 2], vec[k + 3] = np.cumsum(np.abs(tx), dtype=F)[-1], np.cumsum(np.abs(ty), dtype=F)[-1]
    mag = np.cumsum((vec * vec).astype(np.float64))[-1]
    with np.errstate(all="ignore"):
        return vec * F(1.0 / (math.sqrt(mag) + np.finfo(np.float64).eps)), band


def detect(img, threshold=600.0, n_octaves=2, n_layers=2):
    """every refined maximum, in the total order"""
    return sorted(maxima(layers(integral(img), n_octaves, n_layers), threshold, n_layers), key=order_key)


def extract(img, disp=None, threshold=600.0, n_octaves=2, n_layers=2, max_keypoints=None):
    """dict: kp (KP_DTYPE), uvu [n][3] f64, desc [n][64] f32, band [n] bool, alt_angle [n] f32, n_maxima, overflow"""
    img = np.ascontiguousarray(img, np.uint8)
    S = integral(img)
    cands = sorted(maxima(layers(S, n_octaves, n_layers), threshold, n_layers), key=order_key)
    n_max = len(cands)
    if max_keypoints is not None:
        cands = cands[:max_keypoints]
    kps, uvu, desc, band, alt = [], [], [], [], []
    for c in cands:
        u = np.array([float(c["x"]), float(c["y"]), float(c["x"])]) if disp is None else disparity_rule(disp, c["x"], c["y"])
        if u is None:
            continue
        o = orientation(S, c)
        if o is None:
            continue
        ang, d, al, bd = o
        v, bd2 = descriptor(img, c, d)
        kps.append((c["x"], c["y"], c["size"], ang, c["response"], c["octave"], c["laplacian"], 0))
        uvu.append(u), desc.append(v), band.append(bd or bd2), alt.append(al)
    n = len(kps)
    return dict(kp=np.array(kps, KP_DTYPE) if n else np.zeros(0, KP_DTYPE), uvu=np.array(uvu, np.float64).reshape(n, 3), desc=np.array(desc, F).reshape(n, 64),
                band=np.array(band, bool), alt_angle=np.array(alt, F), n_maxima=n_max, overflow=max_keypoints is not None and n_max > max_keypoints)


# ---- the test images --------------------------------------------------------------------------------------------------------------------------------------------
def blob_image(w, h, seed, n_blobs=None, sigma=(2.0, 8.0)):
    """a seeded sum of Gaussian blobs of sigma 2 .. 8 px plus mild noise, quantised to u8"""
    rng = np.random.default_rng(seed)
    n = n_blobs or max(40, w * h // 90)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.full((h, w), 110.0)
    for _ in range(n):
        cx, cy, sg, amp = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(*sigma), rng.uniform(40, 120) * rng.choice([-1, 1])
        im += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sg * sg))
    im += rng.normal(0, 1.5, (h, w))
    return np.clip(np.rint(im), 0, 255).astype(np.uint8)


def disparity_field(w, h, seed):
    """a seeded field with a zero / negative region and a +inf patch"""
    rng = np.random.default_rng(seed + 1000)
    d = rng.uniform(2.0, 30.0, (h, w)).astype(F)
    d[:h // 5, :w // 3] = 0
    d[h // 5:h // 4, :w // 3] = -1
    d[h // 2:h // 2 + 6, w // 2:w // 2 + 8] = np.inf
    return d


# the images of the device tests, in ONE place (tests/test_gpu_surf.py, tests/test_surf_cpu.py and the band statistics of tools/time_surf.py):
# name -> (w, h, seed, n_blobs, sigma range).  Seeds chosen on this model alone so that the bands hold at most 10 % of the keypoints and leave at least 20 outside
TEST_IMAGES = {"160x120": (160, 120, 6, None, (2.0, 8.0)), "97x75": (97, 75, 1, 120, (2.0, 3.5)), "256x192": (256, 192, 4, None, (2.0, 8.0)),
               "128x96-a": (128, 96, 8, None, (2.0, 8.0)), "128x96-b": (128, 96, 1, None, (2.0, 8.0))}


def test_image(name):
    """(image, disparity) of TEST_IMAGES[name]"""
    w, h, seed, nb, sg = TEST_IMAGES[name]
    return blob_image(w, h, seed, nb, sg), disparity_field(w, h, seed)


test_image.__test__ = False      # (a helper, not a test)


def shifted_pair(w=256, h=192, dx=8, dy=4, seed=4):
    """two w x h windows of one larger image: the content at (x, y) of the first lies at (x + dx, y + dy) of the second.  No wrap; dx, dy multiples of every
    octave's step, so the sample grids of both windows fall on the same pixels of the content and the keypoints correspond up to the f32 rounding of x + dx"""
    big = blob_image(w + dx, h + dy, seed)
    return np.ascontiguousarray(big[dy:dy + h, dx:dx + w]), np.ascontiguousarray(big[:h, :w])
