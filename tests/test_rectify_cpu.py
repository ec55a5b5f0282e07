"""The rectifier's semantics (tests/rectify_model.py) against properties that do not come from the model, and the library's host-side map builder
(svs_rectify_build_maps) against the model in every entry.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import rectify_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _identity_maps(w, h, dx=0, dy=0, frac=0):
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    return np.stack([jj + dx, ii + dy], axis=-1).astype(np.int16), np.full((h, w), frac, np.uint16)


def _img(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# ---- the model against properties that are not the model ----------------------------------------------------------------------------------------------
def test_identity_map_returns_the_image():
    img = _img(96, 40, 1)
    xy, fr = _identity_maps(96, 40)
    assert np.array_equal(RM.remap(img, xy, fr), img)


def test_integer_shift_map_shifts_with_zero_fill():
    img = _img(96, 40, 2)
    for dx, dy in ((5, 0), (-7, 3), (0, -4), (11, 9)):
        xy, fr = _identity_maps(96, 40, dx, dy)
        want = np.zeros_like(img)
        ys, xs = np.arange(40) + dy, np.arange(96) + dx
        oky, okx = (ys >= 0) & (ys < 40), (xs >= 0) & (xs < 96)
        want[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
        assert np.array_equal(RM.remap(img, xy, fr), want), (dx, dy)


def test_half_pixel_in_x_is_the_rounded_mean():
    img = _img(96, 40, 3)
    xy, fr = _identity_maps(96, 40, frac=16)      # fx = 16, fy = 0
    a = img.astype(np.int64)
    b = np.zeros_like(a); b[:, :-1] = a[:, 1:]    # the right neighbour; outside the image reads 0
    assert np.array_equal(RM.remap(img, xy, fr), ((a + b + 1) >> 1).astype(np.uint8))


def test_gray_of_white_and_coefficient_sum():
    assert RM.GRAY_B + RM.GRAY_G + RM.GRAY_R == 16384
    assert RM.bgr_to_gray(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255
    assert RM.bgr_to_gray(np.zeros((1, 1, 3), np.uint8))[0, 0] == 0
    for v in (1, 17, 128, 254):                    # a gray BGR pixel keeps its value
        assert RM.bgr_to_gray(np.full((1, 1, 3), v, np.uint8))[0, 0] == v


def test_fixed_point_is_the_exact_bilinear_value_rounded_once():
    """|fixed - float bilinear at the quantised coordinates| <= 0.5: the weights are exact multiples of 1/1024 that sum to 1, so the accumulator IS the exact
    value times 1024 and `(acc + 512) >> 10` rounds it once"""
    rng = np.random.default_rng(4)
    w, h = 80, 60
    img = _img(w, h, 5)
    xy = np.stack([rng.integers(-2, w + 1, (h, w)), rng.integers(-2, h + 1, (h, w))], axis=-1).astype(np.int16)
    fr = rng.integers(0, 1024, (h, w)).astype(np.uint16)
    got = RM.remap(img, xy, fr).astype(np.float64)
    pad = np.zeros((h + 6, w + 6)); pad[3:3 + h, 3:3 + w] = img
    x0, y0 = xy[..., 0].astype(int) + 3, xy[..., 1].astype(int) + 3
    ax, ay = (fr & 31) / 32.0, (fr >> 5) / 32.0
    exact = (1 - ay) * ((1 - ax) * pad[y0, x0] + ax * pad[y0, x0 + 1]) + ay * ((1 - ax) * pad[y0 + 1, x0] + ax * pad[y0 + 1, x0 + 1])
    assert np.abs(got - exact).max() <= 0.5


def test_fused_colour_and_remap_equals_gray_then_remap():
    rng = np.random.default_rng(6)
    bgr = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    xy = np.stack([rng.integers(-2, 65, (48, 64)), rng.integers(-2, 49, (48, 64))], axis=-1).astype(np.int16)
    fr = rng.integers(0, 1024, (48, 64)).astype(np.uint16)
    assert np.array_equal(RM.rectify(bgr, xy, fr), RM.remap(RM.bgr_to_gray(bgr), xy, fr))


def test_depth_model_zero_is_inf_and_one_metre():
    d = RM.depth_to_disp(np.array([0, 5000], np.uint16), 525.0, 0.075)
    assert np.isposinf(d[0]) and abs(d[1] - 525.0 / 0.075) < 1e-2


# ---- the library's map builder against the model -------------------------------------------------------------------------------------------------------
def _lib_build_maps(K, dist, R, Knew, w, h):
    from scavislam_amd import capi
    lib = capi.load()
    K, R, Knew = (np.ascontiguousarray(a, np.float64).reshape(9) for a in (K, R, Knew))
    dist = np.ascontiguousarray(dist, np.float64)
    xy, fr = np.zeros((h, w, 2), np.int16), np.zeros((h, w), np.uint16)
    rc = lib.svs_rectify_build_maps(K.ctypes.data, dist.ctypes.data, R.ctypes.data, Knew.ctypes.data, w, h, xy.ctypes.data, fr.ctypes.data)
    assert rc == 0
    return xy, fr


@pytest.mark.parametrize("lens", list(RM.LENS_SETS))
@pytest.mark.parametrize("camera", list(RM.CAMERAS))
def test_build_maps_equals_the_model_in_every_entry(camera, lens):
    w, h, f, cx, cy = RM.CAMERAS[camera]
    dist, rv = RM.LENS_SETS[lens]
    K, R = RM.intrinsics(f, cx, cy), RM.rodrigues(rv)
    xy, fr = _lib_build_maps(K, dist, R, K, w, h)
    xy_m, fr_m = RM.build_maps(K, dist, R, K, w, h)
    assert np.array_equal(xy, xy_m) and np.array_equal(fr, fr_m)
    assert fr.max() <= 1023
    if lens == "zero":                              # no distortion, no rotation: the identity map
        xy_i, fr_i = _identity_maps(w, h)
        assert np.array_equal(xy, xy_i) and np.array_equal(fr, fr_i)
    else:
        assert not np.array_equal(xy, _identity_maps(w, h)[0])


def test_build_maps_rejects_null_and_singular():
    from scavislam_amd import capi
    lib = capi.load()
    K = np.ascontiguousarray(RM.intrinsics(100.0, 8.0, 8.0)).reshape(9)
    Z, d = np.zeros(9), np.zeros(5)
    xy, fr = np.zeros((16, 16, 2), np.int16), np.zeros((16, 16), np.uint16)
    assert lib.svs_rectify_build_maps(None, d.ctypes.data, K.ctypes.data, K.ctypes.data, 16, 16, xy.ctypes.data, fr.ctypes.data) == 1
    assert lib.svs_rectify_build_maps(K.ctypes.data, d.ctypes.data, Z.ctypes.data, K.ctypes.data, 16, 16, xy.ctypes.data, fr.ctypes.data) == 1


def test_python_frame_grabber_builds_the_model_maps():
    """the FrameGrabber mirror's intializeRectifier (Rodrigues on the host, Knew = K) without a device"""
    from scavislam_amd.frontend import FrameGrabber
    w, h, f, cx, cy = RM.CAMERAS["320x240"]
    dist, rv = RM.LENS_SETS["first"]
    cam = dict(f=f, cx=cx, cy=cy, b=0.1, w=w, h=h)
    xy, fr = FrameGrabber.build_maps(cam, rv, dist)
    K = RM.intrinsics(f, cx, cy)
    xy_m, fr_m = RM.build_maps(K, dist, RM.rodrigues(rv), K, w, h)
    assert np.array_equal(xy, xy_m) and np.array_equal(fr, fr_m)


def test_cpp_rectifier_class_compiles(tmp_path):
    """FrameRectifier of include/scavislam_hip.hpp with plain g++; its Rodrigues + map builder run without a device and give the model's maps"""
    src = tmp_path / "r.cpp"
    src.write_text('#include "scavislam_hip.hpp"\n'
                   'int main(){ double R[9]; const double rv[3] = {0.004, -0.011, 0.007}; scavislam_hip::FrameRectifier::rodrigues(rv, R);\n'
                   '  const double K[9] = {265.0, 0, 159.5, 0, 265.0, 119.5, 0, 0, 1}; const double d[5] = {-0.28, 0.07, 1e-3, -5e-4, 0.01};\n'
                   '  std::vector<int16_t> xy(2 * 320 * 240); std::vector<uint16_t> fr(320 * 240);\n'
                   '  if (svs_rectify_build_maps(K, d, R, K, 320, 240, xy.data(), fr.data()) != SVS_OK) return 1;\n'
                   '  std::fwrite(R, 8, 9, stdout); std::fwrite(xy.data(), 2, xy.size(), stdout); std::fwrite(fr.data(), 2, fr.size(), stdout);\n'
                   '  scavislam_hip::Context c(0); if (!c.ok()) return 0;\n'
                   '  svs_cam cam = {265.0, 159.5, 119.5, 0.1, 320, 240}; scavislam_hip::FrameRectifier g(c, cam, 2);\n'
                   '  return g.intializeRectifier(rv, d, rv, d) ? 0 : 2; }\n')
    exe = tmp_path / "r"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.check_output([str(exe)])
    n = 320 * 240
    R = np.frombuffer(out[:72], np.float64).reshape(3, 3)
    xy = np.frombuffer(out[72:72 + 4 * n], np.int16).reshape(240, 320, 2)
    fr = np.frombuffer(out[72 + 4 * n:72 + 6 * n], np.uint16).reshape(240, 320)
    w, h, f, cx, cy = RM.CAMERAS["320x240"]
    dist, rv = RM.LENS_SETS["first"]
    assert np.abs(R - RM.rodrigues(rv)).max() < 1e-15      # (libm's sin / cos: the last bit is not the header's to promise)
    K = RM.intrinsics(f, cx, cy)
    xy_m, fr_m = RM.build_maps(K, dist, R, K, w, h)
    assert np.array_equal(fr, fr_m) and np.array_equal(xy, xy_m)
