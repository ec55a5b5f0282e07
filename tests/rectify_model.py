"""NumPy model of the arithmetic between the camera and processFrame (FrameGrabber::processNextFrame, frame_grabber.cpp:125-186): colour to gray
(cv::cvtColor CV_BGR2GRAY), rectification (cv::remap CV_INTER_LINEAR on CV_16SC2 maps, BORDER_CONSTANT 0), the map builder
(cv::initUndistortRectifyMap) and depth to disparity (frame_grabber-impl.cpp:136-152, stereo_camera.cpp:55-59).

OpenCV is not available to the tests: like FAST, pyrDown and StereoBM these are restated from OpenCV 2.4's published algorithms and are NOT pinned by
the reference's binaries.  The operation order written here is the definition the library is held to, bit for bit."""
import numpy as np

GRAY_B, GRAY_G, GRAY_R = 1868, 9617, 4899      # 14-bit fixed point of 0.114, 0.587, 0.299


def bgr_to_gray(bgr):
    """[h, w, 3] u8 (B, G, R interleaved) -> [h, w] u8"""
    p = np.asarray(bgr).astype(np.int64)
    return ((GRAY_B * p[..., 0] + GRAY_G * p[..., 1] + GRAY_R * p[..., 2] + 8192) >> 14).astype(np.uint8)


def tap_coords(map_xy):
    """x, y of the four taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) as int64 [4][h][w]"""
    x0 = map_xy[..., 0].astype(np.int64)
    y0 = map_xy[..., 1].astype(np.int64)
    return np.stack([x0, x0 + 1, x0, x0 + 1]), np.stack([y0, y0, y0 + 1, y0 + 1])


def taps_inside(map_xy, w, h):
    """bool [4][h][w]: which taps lie inside a w x h source"""
    xs, ys = tap_coords(map_xy)
    return (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)


def remap(src, map_xy, map_frac):
    """src [hs, ws] u8; map_xy [h, w, 2] int16; map_frac [h, w] uint16 (fx = frac & 31, fy = frac >> 5) -> [h, w] u8.  A tap outside reads 0, per tap"""
    src = np.asarray(src)
    hs, ws = src.shape
    xs, ys = tap_coords(map_xy)
    ok = taps_inside(map_xy, ws, hs)
    p = np.where(ok, src[np.clip(ys, 0, hs - 1), np.clip(xs, 0, ws - 1)].astype(np.int64), 0)
    frac = np.asarray(map_frac).astype(np.int64)
    assert frac.max(initial=0) <= 1023
    fx, fy = frac & 31, frac >> 5
    acc = (32 - fx) * (32 - fy) * p[0] + fx * (32 - fy) * p[1] + (32 - fx) * fy * p[2] + fx * fy * p[3] + 512
    return (acc >> 10).astype(np.uint8)


def rectify(raw, map_xy=None, map_frac=None):
    """what one side of the rectifier produces: raw [h, w] gray or [h, w, 3] BGR; maps None = conversion / copy only"""
    g = bgr_to_gray(raw) if np.asarray(raw).ndim == 3 else np.asarray(raw, np.uint8)
    return g.copy() if map_xy is None else remap(g, map_xy, map_frac)


def rodrigues(rv):
    """rotation vector -> R (SO3::exp)"""
    rv = np.asarray(rv, np.float64)
    th = float(np.sqrt(rv @ rv))
    Kx = np.array([[0.0, -rv[2], rv[1]], [rv[2], 0.0, -rv[0]], [-rv[1], rv[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + Kx
    return np.eye(3) + (np.sin(th) / th) * Kx + ((1.0 - np.cos(th)) / (th * th)) * (Kx @ Kx)


def intrinsics(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


def build_maps(K, dist, R, Knew, w, h):
    """cv::initUndistortRectifyMap(K, dist, R, Knew, (w, h), CV_16SC2): f64, no contraction, the operation order below IS the definition.
    dist = (k1, k2, p1, p2, k3).  Returns map_xy int16 [h, w, 2], map_frac uint16 [h, w]"""
    K, R, Kn = (np.asarray(a, np.float64).reshape(3, 3) for a in (K, R, Knew))
    k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
    M = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            M[r, c] = (Kn[r, 0] * R[0, c] + Kn[r, 1] * R[1, c]) + Kn[r, 2] * R[2, c]
    (a, b, c), (d, e, f), (g, hh, i) = M
    A, B, Cc = e * i - f * hh, c * hh - b * i, b * f - c * e
    D, E, F = f * g - d * i, a * i - c * g, c * d - a * f
    G, H, I = d * hh - e * g, b * g - a * hh, a * e - b * d
    det = (a * A + b * D) + c * G
    iR = np.array([[A, B, Cc], [D, E, F], [G, H, I]]) / det
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = (jj * iR[0, 0] + ii * iR[0, 1]) + iR[0, 2]
    Y = (jj * iR[1, 0] + ii * iR[1, 1]) + iR[1, 2]
    W = (jj * iR[2, 0] + ii * iR[2, 1]) + iR[2, 2]
    x, y = X / W, Y / W
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    _2xy = (2.0 * x) * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    fx, fy, u0, v0 = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    u = fx * ((x * kr + p1 * _2xy) + p2 * (r2 + 2.0 * x2)) + u0
    v = fy * ((y * kr + p1 * (r2 + 2.0 * y2)) + p2 * _2xy) + v0
    iu = np.rint(u * 32.0).astype(np.int64)
    iv = np.rint(v * 32.0).astype(np.int64)
    map_xy = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], axis=-1)
    map_frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map_xy, map_frac


def depth_to_disp(d16, f, b):
    """FrameGrabber<StereoCamera>::depthToDisp: float depth = d16 * (float)(1./5000.); StereoCamera::depthToDisp(depth) with double f, b.
    d16 == 0 gives +inf, as the reference does"""
    depth = np.asarray(d16, np.uint16).astype(np.float32) * np.float32(1. / 5000.)
    with np.errstate(divide="ignore"):
        sd = (np.float64(f) / depth.astype(np.float64)).astype(np.float32)
        return (sd.astype(np.float64) / np.float64(b)).astype(np.float32)


# the lens sets the tests use: (dist, rotation vector)
LENS_SETS = {
    "first": ((-0.28, 0.07, 1e-3, -5e-4, 0.01), (0.004, -0.011, 0.007)),
    "second": ((-0.25, 0.05, -8e-4, 6e-4, 0.0), (-0.003, 0.009, -0.02)),
    "zero": ((0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "harsh": ((0.35, 0.2, 5e-3, 5e-3, 0.0), (0.05, -0.06, 0.09)),
}
# (w, h, f, cx, cy): 640 x 480, New College's camera, 320 x 240
CAMERAS = {
    "640x480": (640, 480, 530.0, 319.5, 239.5),
    "512x384": (512, 384, 389.956, 254.903, 201.899),
    "320x240": (320, 240, 265.0, 159.5, 119.5),
}
