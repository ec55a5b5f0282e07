"""svs_surf_extract / svs_loop_set_place_from_surf (SURF detection, the disparity filter and description on the device) against the restatement tests/surf_model.py.

Bounds.  Everything up to the keypoint list is integer or f32 arithmetic in a fixed order: count, order, positions, sizes, responses, laplacian signs, the kept
set and uvu must be EQUAL as bits.  Angles and descriptors go through atan2 / sin / cos, which both sides take in f64 and round to f32: outside the model's
bands (surf_model.py: exactly as wide as one f32 ulp of those functions can reach) they must be EQUAL as bits too; inside, the angle is one of the model's two
candidates and the descriptor is held to unit norm.  The bands may hold at most 10 % of an image's keypoints and must leave at least 20 outside (asserted; the
seeds were chosen on the model alone).  The band widths are NARROWER than a blanket 1e-3 degrees / 1e-4 px, which would hold most keypoints of any image (a window
has up to 2 x 151^2 coordinates): narrower bands hold more keypoints to bit equality."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import loop_model as L
import surf_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = dict(f=200.0, cx=80.0, cy=60.0, b=0.12)
# image of surf_model.TEST_IMAGES: device row stride
CASES = {"160x120": 160, "97x75": 128, "256x192": 256}
BATCH = ["128x96-a", "128x96-b", None]      # None: the all-zero image


@pytest.fixture(scope="module")
def ctx():
    from scavislam_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(name):
    img, disp = M.test_image(name)
    return img, disp, M.extract(img, disp), CASES[name]


@functools.lru_cache(maxsize=None)
def batch_case():
    pairs = [(np.zeros((96, 128), np.uint8), M.disparity_field(128, 96, 0)) if c is None else M.test_image(c) for c in BATCH]
    imgs, disp = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return imgs, disp, [M.extract(imgs[k], disp[k]) for k in range(3)]


def extractor(ctx, w, h, **kw):
    from scavislam_amd.loop import SurfExtractor
    return SurfExtractor(ctx, CAM, w, h, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_band_cap(m):
    n, b = len(m["kp"]), int(m["band"].sum())
    assert b <= 0.1 * n and n - b >= 20, (n, b)


def assert_equals_model(out, m, cap=True):
    print("keypoints", len(out), "model", len(m["kp"]), "maxima", m["n_maxima"], "in bands", int(m["band"].sum()))
    if cap:
        assert_band_cap(m)
    assert len(out) == len(m["kp"])
    for f in ("x", "y", "size", "response", "octave", "laplacian"):
        assert np.array_equal(bits(out.keypoints[f]), bits(m["kp"][f])), f
    assert np.array_equal(out.uvu.view(np.uint64), m["uvu"].view(np.uint64))
    free = ~m["band"]
    bad_a = int((bits(out.keypoints["angle"]) != bits(m["kp"]["angle"]))[free].sum())
    bad_d = int((bits(out.descriptors) != bits(m["desc"])).any(1)[free].sum())
    print("outside the bands: angles differing", bad_a, "descriptors differing", bad_d)
    assert bad_a == 0 and bad_d == 0
    a = out.keypoints["angle"][m["band"]]
    assert ((bits(a) == bits(m["kp"]["angle"][m["band"]])) | (bits(a) == bits(m["alt_angle"][m["band"]]))).all()
    if len(out):
        assert np.abs(np.linalg.norm(out.descriptors.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert out.overflow == m["overflow"]


def raw_bytes(ex, b=0):
    n = ex.raw["count"][b]
    return [ex.raw["count"][b:b + 1].tobytes(), ex.raw["overflow"][b:b + 1].tobytes()] + [ex.raw[k][b, :n].tobytes() for k in ("keypoints", "uvu", "descriptors")]


# ---- 1. parity with the model -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_model(ctx, name):
    img, disp, m, stride = case(name)
    h, w = img.shape
    ex = extractor(ctx, w, h)
    out = ex.extract(img[None], disp[None], stride=stride)[0]
    assert_equals_model(out, m)
    first = raw_bytes(ex)
    ex.extract(img[None], disp[None], stride=stride)
    assert raw_bytes(ex) == first                              # a repetition: byte for byte
    ex.close()


def test_batch_equals_alone_at_any_stride(ctx):
    imgs, disp, ms = batch_case()
    ex = extractor(ctx, 128, 96, max_batch=3)
    outs = ex.extract(imgs, disp)
    in_batch = [raw_bytes(ex, k) for k in range(3)]
    for k in range(3):
        assert_equals_model(outs[k], ms[k], cap=BATCH[k] is not None)
    assert len(outs[2]) == 0 and not outs[2].overflow          # the all-zero image
    for k in range(3):
        ex.extract(imgs[k:k + 1], disp[k:k + 1])
        assert raw_bytes(ex) == in_batch[k], k                 # alone
        ex.extract(imgs[k:k + 1], disp[k:k + 1], stride=173)
        assert raw_bytes(ex) == in_batch[k], k                 # at another stride
    ex.extract(imgs[::-1].copy(), disp[::-1].copy())
    assert [raw_bytes(ex, 2 - k) for k in range(3)] == in_batch      # in another place of the batch
    ex.close()


def test_without_disparity(ctx):
    from scavislam_amd.ctypes_types import SurfParams
    img, _, _, _ = case("160x120")
    m = M.extract(img, None)
    ex = extractor(ctx, 160, 120, params=SurfParams.reference(require_disparity=False))
    assert_equals_model(ex.extract(img[None])[0], m, cap=False)
    ex.close()


# ---- 2. more maxima than max_keypoints --------------------------------------------------------------------------------------------------------------------------
def test_overflow_keeps_the_strongest(ctx):
    img, disp, m, _ = case("160x120")
    assert m["n_maxima"] > 16
    mt = M.extract(img, disp, max_keypoints=16)
    ex = extractor(ctx, 160, 120, max_keypoints=16)
    out = ex.extract(img[None], disp[None])[0]
    assert out.overflow and mt["overflow"]
    assert_equals_model(out, mt, cap=False)
    n = len(out)
    assert 0 < n <= 16
    full = extractor(ctx, 160, 120)
    f = full.extract(img[None], disp[None])[0]
    assert not f.overflow
    assert out.keypoints.tobytes() == f.keypoints[:n].tobytes() and out.descriptors.tobytes() == f.descriptors[:n].tobytes()      # the strongest prefix of the full run
    ex.close(), full.close()


# ---- 3. the place goes to the loop handle on the device -----------------------------------------------------------------------------------------------------------
def test_place_from_surf_equals_set_place(ctx):
    """An image against a shifted copy of itself (surf_model.shifted_pair: two windows of one larger image, the shift a multiple of every octave's step, so the
    keypoints of the two correspond up to the f32 rounding of x + dx).  The slots loaded device to device and through svs_loop_set_place give identical bytes;
    the check finds the shift's translation to the 1e-6 px that tests/test_gpu_loop.py holds its poses to.  Positions are f32: a matched pair may differ from
    the exact shift by half an ulp at 256 (1.5e-5 px; measured 7.6e-6), and a pose fitted to three such pairs reprojects up to 5e-6 px off the pure shift
    (seeds 4, 5 on the model).  The seed is one where the three matches of the model's best hypothesis round alike in both windows -- a PRECONDITION asserted
    below on the keypoint positions, which the parity tests hold EQUAL to the model's."""
    from scavislam_amd.loop import GeometricChecker
    dx, dy, d0 = 8, 4, 16.0
    img, shifted = M.shifted_pair(256, 192, dx, dy, seed=7)
    disp = np.full((2, 192, 256), d0, np.float32)
    cam = dict(f=250.0, cx=128.0, cy=96.0, b=0.12)
    ex = extractor(ctx, 256, 192, max_batch=2)
    pl = ex.extract(np.stack([img, shifted]), disp)
    gc = GeometricChecker(ctx, cam, desc_dim=64, max_desc=512, max_places=4, max_hyp=100, max_checks=2)
    for k in range(2):
        gc.set_place_from_surf(k, ex, k)
        gc.set_place(2 + k, pl[k].descriptors, pl[k].uvu)
    a = gc.check_batch([(0, 1), (1, 0)], seed=5)
    raw_a = {k: (v if isinstance(v, bytes) else v.tobytes()) for k, v in gc.raw.items()}
    gc.check_batch([(2, 3), (3, 2)], seed=5)
    raw_b = {k: (v if isinstance(v, bytes) else v.tobytes()) for k, v in gc.raw.items()}
    assert raw_a == raw_b                                      # bit-identical both ways
    t = np.array([dx, dy, 0.0]) * cam["b"] / d0                # a pixel shift at constant disparity is a translation by shift * z / f = shift * b / d
    for out, sign in ((a[0], -1.0), (a[1], 1.0)):
        q, tr = (0, 1) if sign < 0 else (1, 0)
        xt = L.unmap_uvu(cam, pl[tr].uvu)
        # the model's RANSAC on the device's matches and samples: the same hypothesis wins, and its three matches are exact correspondences (the precondition)
        m = L.ransac(cam, pl[q].uvu, xt, out.train_idx, out.samples, 2.5)
        assert np.nanmin(np.abs(m["res_final"] - 2.5)) > 1e-6, "precondition: a residual within 1e-6 of the threshold (change the seed)"
        assert (out.best_hyp, out.n_inliers) == (m["best"], m["n_inliers"])
        r = out.samples[out.best_hyp]
        assert np.array_equal(pl[q].uvu[r, :2], pl[tr].uvu[out.train_idx[r], :2] + sign * np.array([dx, dy])), "precondition: the best triple rounds alike (change the seed)"
        # SURF itself: every inlier pair is the shift up to the f32 rounding of a coordinate below 256 (half an ulp = 2^-16 px)
        dev = np.abs(pl[q].uvu[:, :2] - (pl[tr].uvu[out.train_idx, :2] + sign * np.array([dx, dy]))).max(1)
        print("inliers", out.n_inliers, "of", out.n_matches, "worst deviation of an inlier pair from the shift", dev[out.inlier].max())
        assert out.n_inliers > 30 and dev[out.inlier].max() <= 2.0 ** -16
        # the pose: the shift's translation, to the tolerance tests/test_gpu_loop.py uses for its poses
        T = out.T_query_from_train
        err = np.abs(L.map_uvu(cam, xt @ T[:, :3].T + T[:, 3]) - L.map_uvu(cam, xt + sign * t)).max()
        print("t", T[:, 3], "expected", sign * t, "reprojection difference to the pure shift", err)
        assert err < 1e-6
    from scavislam_amd.capi import SvsError
    for bad in (lambda: gc.set_place_from_surf(0, ex, 2), lambda: gc.set_place_from_surf(4, ex, 0)):
        with pytest.raises(SvsError) as e:
            bad()
        assert str(e.value).startswith("status 1:")
    small = GeometricChecker(ctx, cam, desc_dim=64, max_desc=8, max_places=1, max_hyp=100, max_checks=1)
    with pytest.raises(SvsError) as e:
        small.set_place_from_surf(0, ex, 0)
    assert str(e.value).startswith("status 4:")                # n > max_desc, as svs_loop_set_place
    ex.extract(np.zeros((1, 192, 256), np.uint8), disp[:1])
    with pytest.raises(SvsError) as e:
        gc.set_place_from_surf(0, ex, 0)
    assert str(e.value).startswith("status 1:")                # n = 0, as svs_loop_set_place
    small.close(), gc.close(), ex.close()


def test_image_to_candidate_end_to_end(ctx):
    from scavislam_amd.loop import GeometricChecker, train_vocabulary
    imgs = np.stack([M.blob_image(160, 120, s) for s in (2, 3, 4, 2)])      # the fourth repeats the first
    disp = np.full((4, 120, 160), 12.0, np.float32)
    ex = extractor(ctx, 160, 120, max_batch=4)
    pl = ex.extract(imgs, disp)
    assert min(len(p) for p in pl) >= 20
    voc = train_vocabulary(ctx, np.concatenate([p.descriptors for p in pl[:3]]), 64, seed=1)
    gc = GeometricChecker(ctx, CAM, desc_dim=64, max_desc=256, max_places=4, max_hyp=100, max_checks=4)
    gc.set_vocabulary(voc.words)
    for k in range(4):
        gc.set_place_from_surf(k, ex, k)
    locs = gc.add_locations([0, 1, 2, 3], radius=float("inf"))
    print("scores of the fourth location", locs[3].scores, "best", locs[3].best_slot, locs[3].best_score)
    assert locs[3].best_slot == 0
    out = gc.check(3, 0)
    assert out.n_inliers > 30
    gc.close(), ex.close()


# ---- 4. the C++ adaptor -----------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_adaptor_prints_the_same_places(ctx, tmp_path):
    from scavislam_amd.loop import GeometricChecker
    exe = tmp_path / "surf_smoke"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "surf_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    img, _, _, _ = case("160x120")
    imgs = np.stack([img, np.roll(img, (2, 5), axis=(0, 1))])
    disp = np.full((2, 120, 160), 12.0, np.float32)
    with open(tmp_path / "surf.bin", "wb") as f:
        f.write(np.array([160, 120], np.int32).tobytes())
        f.write(np.array([CAM["f"], CAM["cx"], CAM["cy"], CAM["b"]], np.float64).tobytes())
        for k in range(2):
            f.write(imgs[k].tobytes())
            f.write(disp[k].tobytes())
    lines = [l.split() for l in subprocess.check_output([str(exe), str(tmp_path / "surf.bin")]).decode().splitlines()]
    ex = extractor(ctx, 160, 120, max_batch=2, max_keypoints=1024)
    pl = ex.extract(imgs, disp)
    gc = GeometricChecker(ctx, CAM, desc_dim=64, max_desc=1024, max_places=2, max_hyp=100, max_checks=1)
    for k in range(2):
        gc.set_place_from_surf(k, ex, k)
        assert [int(t) for t in next(l for l in lines if l[0] == "PLACE" and int(l[1]) == k)[2:]] == [len(pl[k]), int(pl[k].overflow)]
        rows = [l[2:] for l in lines if l[0] == "KP" and int(l[1]) == k]
        kp = pl[k].keypoints
        want = [["%08x" % bits(kp[f][i:i + 1])[0] for f in ("x", "y", "size", "angle", "response")] + [str(kp["octave"][i]), str(kp["laplacian"][i])] +
                ["%08x" % bits(pl[k].descriptors[i, :1])[0], "%08x" % bits(pl[k].descriptors[i, 63:])[0]] for i in range(len(kp))]
        assert rows == want
    out = gc.check(1, 0, seed=5)
    assert [int(t) for t in next(l for l in lines if l[0] == "LOOP")[1:]] == [int(out.n_inliers > 30), 101, 100, out.n_matches, out.n_inliers]
    gc.close(), ex.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from scavislam_amd.capi import SvsError
    from scavislam_amd.ctypes_types import Cam, SurfParams
    lib = ctx.lib
    live = ctx.get_stat("live_device_bytes")
    cam, prm = Cam(200.0, 80.0, 60.0, 0.12, 0, 0), SurfParams.reference()

    def create(code, w=160, h=120, max_batch=1, max_kp=64, p=prm):
        h_ = C.c_void_p()
        with pytest.raises(SvsError) as e:
            ctx.call("svs_surf_create", C.byref(cam), w, h, max_batch, max_kp, C.byref(p), C.byref(h_))
        assert str(e.value).startswith(f"status {code}:"), str(e.value)
        assert ctx.get_stat("live_device_bytes") == live      # refused before anything was allocated

    create(5, w=53)                                            # smaller than the largest filter (54)
    create(5, h=53)
    create(4, w=4096, h=2057)                                  # w h 255 >= 2^31: the integral image is int32
    create(1, max_batch=0)
    create(1, max_kp=0)
    create(5, p=SurfParams.reference(n_octaves=5))
    create(5, w=1024, h=1024, p=SurfParams.reference(n_octaves=4))      # the largest descriptor window does not fit the LDS
    assert lib.svs_surf_extract(None, None, 0, 0, None, 0, 0, 1, None, None, None, None, None) == 1
    assert lib.svs_loop_set_place_from_surf(None, 0, None, 0) == 1
    assert lib.svs_surf_set_timing(None, 1) == 1 and lib.svs_surf_stage_times(None, None) == 1
    ex = extractor(ctx, 160, 120, max_batch=2)
    img, disp, _, _ = case("160x120")
    with pytest.raises(SvsError) as e:
        ex.extract(np.stack([img] * 3), np.stack([disp] * 3))
    assert str(e.value).startswith("status 4:")                # n_batch > max_batch
    with pytest.raises(SvsError) as e:
        ex.extract(img[None])                                  # require_disparity and no disparity
    assert str(e.value).startswith("status 1:")
    ex.set_timing(True)
    ex.extract(img[None], disp[None])
    ms = ex.stage_times_ms()
    assert len(ms) == 6 and all(v > 0 for v in ms)
    ex.close()
    assert ctx.get_stat("live_device_bytes") == live
