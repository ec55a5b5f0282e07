"""SURF without a device: the properties of the restatement tests/surf_model.py (the yardstick of tests/test_gpu_surf.py), the arithmetic the device compiles
(scavislam_amd/csrc/surf_core.h, run on the host through tests/cpp/surf_host.cpp) against that restatement bit for bit, the seeds of the GPU test against the
band cap, and the exports of the built library."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import surf_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURF_EXPORTS = ["svs_surf_params_default", "svs_surf_create", "svs_surf_destroy", "svs_surf_extract", "svs_loop_set_place_from_surf", "svs_surf_set_timing",
                "svs_surf_stage_times"]
GPU_IMAGES = list(M.TEST_IMAGES)      # the images of tests/test_gpu_surf.py
_model = {}


def model(name):
    if name not in _model:
        img, disp = M.test_image(name)
        _model[name] = (img, disp, M.extract(img, disp))
    return _model[name]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("surf") / "libsurf_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "surf_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.svs_host_surf_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]

    def run(img, disp, max_kp=4096, threshold=600.0, stride=None):
        h, w = img.shape
        st = stride or w
        pad = np.zeros((h, st), np.uint8)
        pad[:, :w] = img
        dp = None
        if disp is not None:
            dp = np.full((h, st), np.nan, np.float32)
            dp[:, :w] = disp
        kp, uvu, desc, nm = np.zeros(max_kp, M.KP_DTYPE), np.zeros((max_kp, 3)), np.zeros((max_kp, 64), np.float32), C.c_int()
        n = lib.svs_host_surf_extract(pad.ctypes.data, st, w, h, None if dp is None else dp.ctypes.data, st, threshold, 2, 2, max_kp, kp.ctypes.data, uvu.ctypes.data,
                                      desc.ctypes.data, C.byref(nm), None, None)
        return kp[:n], uvu[:n], desc[:n], nm.value
    run.lib = lib
    return run


def test_box_sums_equal_direct_sums():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    S = M.integral(img)
    assert S.shape == (38, 54) and (S[0] == 0).all() and (S[:, 0] == 0).all()
    for _ in range(200):
        y1, y2 = sorted(rng.integers(0, 38, 2))
        x1, x2 = sorted(rng.integers(0, 54, 2))
        assert S[y1, x1] + S[y2, x2] - S[y2, x1] - S[y1, x2] == int(img[y1:y2, x1:x2].astype(np.int64).sum())
    # a scaled pattern's value is the weighted sum of its boxes' pixels
    boxes = M.scale_pattern(M.DX, 9, 15)
    assert [b[:4] for b in boxes] == [(0, 3, 5, 12), (5, 3, 10, 12), (10, 3, 15, 12)]
    v = M.haar(S, np.array([4]), np.array([7]), boxes)[0, 0]
    direct = sum(float(np.float32(int(img[4 + y1:4 + y2, 7 + x1:7 + x2].astype(np.int64).sum())) * wt) for (x1, y1, x2, y2, wt) in boxes)
    assert v == np.float32(direct)


def continuous_best_size(sigma):
    """where |Dxx| of the CONTINUOUS box pattern (size L, weights 1 / area), centred on a Gaussian blob of that sigma, peaks: the model of the filter, no image"""
    def phi(a, b):
        return 0.5 * (math.erf(b / (sigma * math.sqrt(2))) - math.erf(a / (sigma * math.sqrt(2))))

    def dxx(L):
        u = L / 9.0
        box = lambda x1, y1, x2, y2: phi((x1 - 4.5) * u, (x2 - 4.5) * u) * phi((y1 - 4.5) * u, (y2 - 4.5) * u)
        return (box(0, 2, 3, 7) - 2 * box(3, 2, 6, 7) + box(6, 2, 9, 7)) / (15 * u * u)
    return max((dxx(L / 50.0) ** 2, L / 50.0) for L in range(450, 3500))[1]


@pytest.mark.parametrize("sigma", [2.8, 4.0, 5.6])
def test_gaussian_blob(sigma):
    w, h, cx, cy = 120, 100, 61.3, 48.6
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.clip(np.rint(40 + 180 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * sigma * sigma))), 0, 255).astype(np.uint8)
    k = M.detect(img)[0]
    assert math.hypot(float(k["x"]) - cx, float(k["y"]) - cy) < 1.0
    # the box filters do not peak at the Gaussian equivalence size 9 sigma / 1.2 but where their own continuous model does (about 5.35 sigma)
    best = continuous_best_size(sigma)
    middle = [(9 + 6 * l) << o for o in range(2) for l in (1, 2)]
    assert (9 + 6 * k["layer"]) << k["octave"] == min(middle, key=lambda s: abs(s - best)), (best, k)
    assert k["laplacian"] == -1                                # a bright blob


def test_rotation_by_90_degrees():
    w = 140
    img = M.blob_image(w, w, 3)
    a, b = M.extract(img), M.extract(np.ascontiguousarray(np.rot90(img)))
    assert len(a["kp"]) >= 30 and len(a["kp"]) == len(b["kp"])
    worst_pos = worst_desc = 0.0
    for i in range(len(a["kp"])):
        k = a["kp"][i]
        d = np.hypot(b["kp"]["x"] - k["y"], b["kp"]["y"] - (w - 1 - k["x"]))      # rot90: (x, y) -> (y, w - 1 - x)
        j = int(np.argmin(d))
        worst_pos = max(worst_pos, float(d[j]))
        da = (float(b["kp"]["angle"][j]) - float(k["angle"]) + 90.0) % 360.0
        assert min(da, 360.0 - da) <= 5.0, (i, da)             # 90 degrees apart, within the window step
        worst_desc = max(worst_desc, float(np.linalg.norm(a["desc"][i].astype(np.float64) - b["desc"][j].astype(np.float64))))
    print("rotation: worst position difference", worst_pos, "worst descriptor distance", worst_desc)
    assert worst_pos < 1e-3
    # measured on the model: 1.3e-4 (profiles/surf.md) -- the box patterns and the sampling grid are symmetric under the rotation of a square image, so the
    # nearest-neighbour window takes the same pixels unless a rounded coordinate flips; one flipped pixel of ~10 grey levels in a patch cell moves a unit
    # descriptor by ~1e-2.  The margin: ten times the measured value
    assert worst_desc < 1.3e-3


def test_unit_norm_and_total_order():
    for spec in GPU_IMAGES[:3]:
        img, disp, m = model(spec)
        assert np.abs(np.linalg.norm(m["desc"].astype(np.float64), axis=1) - 1.0).max() < 1e-6
        c = M.detect(img)
        keys = [M.order_key(k) for k in c]
        assert all(keys[i] < keys[i + 1] for i in range(len(keys) - 1))      # strictly increasing: total, no two equal
        r = [float(k["response"]) for k in c]
        assert r == sorted(r, reverse=True)


def test_disparity_rule():
    disp = np.zeros((20, 30), np.float32)
    disp[5, 11], disp[5, 12], disp[6, 3], disp[7, 3], disp[8, 3] = 4.0, 8.0, -1.0, np.nan, np.inf
    f = np.float32
    assert M.disparity_rule(disp, f(10.5), f(5.0)).tolist() == [10.5, 5.0, 6.5]       # round half away from zero: column 11
    assert M.disparity_rule(disp, f(11.5), f(4.5)).tolist() == [11.5, 4.5, 3.5]       # column 12, row 5 (rint would take 4)
    assert M.disparity_rule(disp, f(12.4), f(5.4))[2] == float(f(12.4)) - 8.0
    assert M.disparity_rule(disp, f(3.0), f(5.0)) is None                             # d = 0
    assert M.disparity_rule(disp, f(3.0), f(6.0)) is None                             # d < 0
    assert M.disparity_rule(disp, f(3.0), f(7.0)) is None                             # NaN
    assert M.disparity_rule(disp, f(3.0), f(8.0))[2] == -np.inf                       # +inf is kept (d > 0)
    assert M.disparity_rule(disp, f(29.5), f(5.0)) is None and M.disparity_rule(disp, f(3.0), f(19.5)) is None      # rounds outside: dropped, never read
    assert M.disparity_rule(disp, f(-0.6), f(5.0)) is None
    disp[9, 3], disp[10, 3] = 1e-20, np.float32(2.0 ** -44)
    assert M.disparity_rule(disp, f(3.0), f(9.0)) is None                             # d > 0 but x - d == x: the place would have uvu[0] - uvu[2] = 0
    assert M.disparity_rule(disp, f(3.0), f(10.0))[2] < 3.0                           # the smallest kind that still separates
    # the filter keeps the order and is a function of the keypoint alone
    img, dsp, m = model(GPU_IMAGES[0])
    every = M.extract(img, None)
    keep = [i for i in range(len(every["kp"])) if M.disparity_rule(dsp, every["kp"]["x"][i], every["kp"]["y"][i]) is not None]
    assert 0 < len(keep) < len(every["kp"])
    assert every["kp"][keep].tobytes() == m["kp"].tobytes() and every["desc"][keep].tobytes() == m["desc"].tobytes()
    assert np.array_equal(m["uvu"][:, 2], m["uvu"][:, 0] - dsp[np.floor(m["uvu"][:, 1] + 0.5).astype(int), np.floor(m["uvu"][:, 0] + 0.5).astype(int)].astype(np.float64))


def test_gpu_test_images_respect_the_band_cap():
    """at most 10 % of an image's keypoints inside the bands, at least 20 outside: checked here, on the model alone"""
    for spec in GPU_IMAGES:
        _, _, m = model(spec)
        n, b = len(m["kp"]), int(m["band"].sum())
        print(spec, "keypoints", n, "maxima", m["n_maxima"], "in bands", b)
        assert b <= 0.1 * n and n - b >= 20, (spec, n, b)


@pytest.mark.parametrize("k", range(3))
def test_device_arithmetic_on_the_host_equals_the_model(host, k):
    """surf_core.h, the arithmetic surf.hip compiles for the device, run as plain loops: every output EQUAL as bits, bands or not (the same libm on both sides)"""
    img, disp, m = model(GPU_IMAGES[k])
    for (d, mm, stride) in ((disp, m, None), (disp, m, img.shape[1] + 31)) + (((None, M.extract(img, None), None),) if k == 0 else ()):
        kp, uvu, desc, n_max = host(img, d, stride=stride)
        assert n_max == mm["n_maxima"] and kp.tobytes() == mm["kp"].tobytes() and uvu.tobytes() == mm["uvu"].tobytes() and desc.tobytes() == mm["desc"].tobytes()
    kp, _, desc, n_max = host(img, disp, max_kp=16)
    mt = M.extract(img, disp, max_keypoints=16)
    assert n_max > 16 and kp.tobytes() == mt["kp"].tobytes() and desc.tobytes() == mt["desc"].tobytes()


def test_host_tables_equal_the_model(host):
    ow, dw = np.zeros(113, np.float32), np.zeros(400, np.float32)
    host.lib.svs_host_surf_tables(C.c_void_p(ow.ctypes.data), C.c_void_p(dw.ctypes.data))
    assert ow.tobytes() == np.array([t[2] for t in M.ORI], np.float32).tobytes() and dw.tobytes() == M.DW.tobytes()
    assert abs(float(M.G_ORI.astype(np.float64).sum()) - 1.0) < 1e-6 and abs(float(M.G_DESC.astype(np.float64).sum()) - 1.0) < 1e-6


def test_exports_exist_in_the_built_library():
    from scavislam_amd import capi
    lib = capi.load()
    for name in SURF_EXPORTS:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    from scavislam_amd.ctypes_types import SurfParams
    p = SurfParams()
    lib.svs_surf_params_default(C.byref(p))
    assert (p.hessian_threshold, p.n_octaves, p.n_octave_layers, p.require_disparity) == (600.0, 2, 2, 1)
    assert lib.svs_surf_extract(None, None, 0, 0, None, 0, 0, 1, None, None, None, None, None) == 1      # no handle: refused before any device call


def test_struct_layouts_match_the_header(tmp_path):
    from scavislam_amd.ctypes_types import SURF_KEYPOINT_DTYPE, SURF_STAGES, SurfParams
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "scavislam_hip.h"\nint main(){printf("%zu %zu %d\\n",sizeof(svs_surf_params),sizeof(svs_surf_keypoint),SVS_SURF_STAGES);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [C.sizeof(SurfParams), SURF_KEYPOINT_DTYPE.itemsize, SURF_STAGES]
    assert SURF_KEYPOINT_DTYPE == M.KP_DTYPE


def test_switched_off_build_keeps_the_exports(tmp_path):
    """make SURF=0: surf.hip compiles to stubs only (host code, no kernel) that still define every export"""
    obj = tmp_path / "surf_off.o"
    subprocess.check_call(["/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-DSVS_NO_SURF",
                           "--cuda-host-only", "-c", os.path.join(ROOT, "scavislam_amd", "csrc", "surf.hip"), "-o", str(obj)])
    syms = subprocess.check_output(["nm", "--defined-only", str(obj)]).decode()
    for name in SURF_EXPORTS:
        assert f" T {name}" in syms, name
    assert "surf_response" not in syms and "surf_describe_kernel" not in syms
