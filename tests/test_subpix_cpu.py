"""The matcher's sub-pixel refinement without a device: the arithmetic the device compiles (scavislam_amd/csrc/subpix_core.h, run on the host through
tests/cpp/subpix_host.cpp) against its definition tests/subpix_model.py bit for bit; the definition against a literal restatement of the reference's dead code
(matcher.cpp:249-304); and the definition against what it is for: sub-pixel positions on a band-limited texture."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import subpix_cases as SC
import subpix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("subpix") / "libsubpix_host.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "cpp", "subpix_host.cpp"), "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.svs_host_subpix.restype = None
    lib.svs_host_subpix.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(K, cimg, disp, lvl, uv, obs, iterations, max_shift, eps):
        n = len(K)
        K, cimg, disp = np.ascontiguousarray(K, np.uint8), np.ascontiguousarray(cimg, np.uint8), np.ascontiguousarray(disp, np.float32)
        uv = np.ascontiguousarray(uv, np.int32)
        status, obs = np.zeros(n, np.int32), np.array(obs, np.float64).reshape(n, 3).copy()
        info_f, info_i = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.int32)
        lib.svs_host_subpix(n, K.ctypes.data, cimg.ctypes.data, cimg.shape[1], cimg.shape[1], cimg.shape[0], disp.ctypes.data, disp.shape[1], lvl, uv.ctypes.data,
                            iterations, max_shift, eps, status.ctypes.data, obs.ctypes.data, info_f.ctypes.data, info_i.ctypes.data)
        info = np.zeros(n, M.INFO_DTYPE)
        info["dx"], info["dy"], info["n_iter"], info["state"] = info_f[:, 0], info_f[:, 1], info_i[:, 0], info_i[:, 1]
        return status, obs, info
    return run


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", SC.GPU_CASES, ids=lambda c: "%s-it%d-s%g-e%g" % c)
def test_core_on_the_host_equals_the_model_on_the_gpu_cases(host, case):
    """Every scene and parameter set of tests/test_gpu_subpix.py: key patches by the model, then subpix_core.h on the host against the model's records and info."""
    name, iterations, max_shift, eps = case
    s = SC.scene(name)
    want, want_info = SC.model(*case)
    ok = np.flatnonzero(s["res"]["status"] == 0)
    assert len(ok) >= 2
    for l in range(3):
        idx = [i for i in ok if s["pts"][i]["anchor_level"] == l]
        if not idx:
            continue
        K = np.stack([M.key_patch(M.affine_inv(s["T_cur_from_w"], s["kf_T"][int(s["pts"][i]["kf_index"])], s["pts"][i], s["cams"][l]), s["pts"][i]["anchor_obs_pyr"][:2],
                                  s["kf_pyr"][int(s["pts"][i]["kf_index"])][l]).reshape(100) for i in idx])
        uv = np.stack([s["res"]["u"][idx], s["res"]["v"][idx]], 1)
        status, obs, info = host(K, s["cur_pyr"][l], s["disp"], l, uv, s["res"]["obs"][idx], iterations, max_shift, eps)
        assert np.array_equal(status, want["status"][idx]), (name, l)
        assert same_bits(obs, np.ascontiguousarray(want["obs"][idx])), (name, l)
        assert same_bits(info, np.ascontiguousarray(want_info[idx])), (name, l)
    print(name, case[1:], "states", np.bincount(want_info["state"], minlength=5), "max |p|", float(max(np.abs(want_info["dx"]).max(), np.abs(want_info["dy"]).max())))


def test_the_gpu_scenes_hold_what_their_names_say():
    """The properties the GPU tests rely on, from the model alone."""
    st = lambda name, *a: SC.model(name, *a)[1]["state"]      # noqa: E731
    for name in ("mixed0", "mixed1", "mixed2", "big"):
        s, i = SC.scene(name), SC.model(name)[1]
        ok = s["res"]["status"] == 0
        assert (i["state"][~ok] == M.UNTOUCHED).all() and (i["state"][ok] != M.UNTOUCHED).all()
        assert (i["state"] == M.REFINED).sum() >= (40 if name == "mixed2" else 8), (name, np.bincount(i["state"]))      # (20 degrees of roll: see subpix_cases)
        assert set(np.unique(s["res"]["status"])) == set(range(8))                        # every status other than OK is there
    s = SC.scene("mixed0")
    assert set(s["pts"]["kf_index"][s["res"]["status"] == 0]) == {0, 1}                   # anchors in two keyframe slots
    assert any((M.key_patch(M.affine_inv(s["T_cur_from_w"], s["kf_T"][int(p["kf_index"])], p, s["cams"][int(p["anchor_level"])]), p["anchor_obs_pyr"][:2],
                            s["kf_pyr"][int(p["kf_index"])][int(p["anchor_level"])]) == 0).any()
               for p in s["pts"][s["res"]["status"] == 0])                                # part of some key patch lies outside the keyframe
    lv = SC.scene("big")["pts"]["anchor_level"]
    assert ((SC.model("big")[1]["state"] == M.REFINED) & (lv == 2)).sum() >= 5              # level 2 refined where the level is large enough
    i8, i8e0 = SC.model("mixed0", 8, 1.5, 0.03)[1], SC.model("mixed0", 8, 1.5, 0.0)[1]
    assert (i8e0["n_iter"][i8e0["state"] == M.REFINED] == 8).all() and (i8["n_iter"][i8["state"] == M.REFINED] < 8).any()      # eps = 0: all iterations run
    for name in ("margin_lo", "margin_hi", "margin_l1"):                                  # taps on the outermost admissible columns / rows: |p| beyond 1
        i = SC.model(name, 8, 2.0, 0.03)[1]
        far = (i["state"] == M.REFINED) & (np.maximum(np.abs(i["dx"]), np.abs(i["dy"])) > 1.0)
        assert far.sum() >= 3, (name, i)
    u2 = SC.model("u2")[1]
    assert list(u2["state"][:4]) == [M.SHIFT] * 4 and (u2["n_iter"][:4] == 0).all() and u2["state"][4] == M.REFINED
    assert (st("flat") == M.SINGULAR).all() and (st("edge") == M.SINGULAR).all()
    far = SC.model("far")[1]
    assert (far["state"] == M.SHIFT).sum() >= 10 and (far["n_iter"][far["state"] == M.SHIFT] >= 1).all()
    h, hi = SC.scene("holes"), SC.model("holes")
    assert h["n_holes"] >= 6 and (hi[1]["state"] == M.NO_DISP).sum() >= 6 and (hi[0]["status"][hi[1]["state"] == M.NO_DISP] == 6).all()
    assert same_bits(np.ascontiguousarray(hi[0]["obs"][hi[1]["state"] == M.NO_DISP]), np.ascontiguousarray(h["res"]["obs"][hi[1]["state"] == M.NO_DISP]))


def _random_records(seed, n):
    """Seeded records of all kinds on one 64 x 48 image: key patches cut from a shifted copy of the texture (converging), from elsewhere (diverging), flat, edges"""
    rng = np.random.default_rng(seed)
    tex = SC.texture(seed)
    ys, xs = np.mgrid[0:48, 0:64].astype(np.float64)
    img = np.clip(np.rint(tex(xs, ys, 1.0)), 0, 255).astype(np.uint8)
    K, uv = np.zeros((n, 10, 10), np.uint8), np.zeros((n, 2), np.int32)
    for r in range(n):
        u, v = int(rng.integers(3, 61)), int(rng.integers(3, 45))
        uv[r] = u, v
        kind = rng.integers(0, 10)
        gy, gx = np.mgrid[0:10, 0:10].astype(np.float64)
        if kind == 0:
            K[r] = rng.integers(0, 256)
        elif kind == 1:
            K[r] = np.where(gx > rng.integers(2, 8), 200, 30)
        elif kind == 2:
            K[r] = rng.integers(0, 256, (10, 10))
        else:
            o = rng.uniform(-2.2, 2.2, 2)
            K[r] = np.clip(np.rint(tex(u - 5 + gx + o[0], v - 5 + gy + o[1], 1.0) + rng.normal(0, 2, (10, 10))), 0, 255)
    disp = np.where(rng.random((48, 64)) < 0.1, rng.choice([0.0, -2.0, np.nan], (48, 64)), 5.0).astype(np.float32)
    return img, disp, K, uv


@pytest.mark.parametrize("lvl, iterations, max_shift, eps", [(0, 8, 1.5, 0.03), (0, 16, 2.0, 0.0), (0, 1, 0.5, 0.5)])
def test_core_on_the_host_equals_the_model_on_seeded_records(host, lvl, iterations, max_shift, eps):
    n = 1000
    img, disp, K, uv = _random_records(100 + iterations, n)
    obs0 = np.random.default_rng(1).normal(size=(n, 3))
    status, obs, info = host(K.reshape(n, 100), img, disp, lvl, uv, obs0, iterations, max_shift, eps)
    states = np.zeros(5, int)
    for r in range(n):
        st, o, i = M.refine_patch(K[r], img, disp, lvl, int(uv[r, 0]), int(uv[r, 1]), obs0[r], iterations, max_shift, eps)
        assert st == status[r] and o.tobytes() == obs[r].tobytes() and i.tobytes() == info[r].tobytes(), (r, st, status[r], o, obs[r], i, info[r])
        states[i["state"]] += 1
    print("states", states)
    assert states[M.REFINED] >= 50 and states[M.SINGULAR] >= 50 and states[M.SHIFT] >= 100 and states[M.NO_DISP] >= 5


def _dead_code(K, cimg, u, v):
    """matcher.cpp:249-304, literally: f32 Sobel (ksize 1, scale 0.5: central differences), warp2d at (0, 0), sequential f32 sums, an f32 LDL^T solve (Eigen's
    ldlt of a 2 x 2 matrix: pivot on the larger diagonal entry)."""
    Kf = K.astype(f32)
    dx, dy = f32(0.5) * (Kf[1:9, 2:10] - Kf[1:9, 0:8]), f32(0.5) * (Kf[2:10, 1:9] - Kf[0:8, 1:9])
    warped = M.current_patch(cimg, u, v, f32(0), f32(0))
    diff = warped - Kf[1:9, 1:9]
    H = np.zeros((2, 2), f32)
    Jres = np.zeros(2, f32)
    for h in range(8):
        for w in range(8):
            J = np.array([dx[h, w], dy[h, w]], f32)
            d = diff[h, w]
            Jres = Jres + J * d
            H = H + np.outer(J, J).astype(f32)
    rhs = -Jres
    p = 0 if H[0, 0] >= H[1, 1] else 1
    q = 1 - p
    with np.errstate(all="ignore"):                 # (a singular H: the caller does not look at the step)
        L = H[q, p] / H[p, p]
        D1 = H[q, q] - L * H[q, p]
        y1 = rhs[q] - L * rhs[p]
        xq = y1 / D1
        xp = rhs[p] / H[p, p] - L * xq
    delta = np.zeros(2, f32)
    delta[p], delta[q] = xp, xq
    return H, Jres, diff, delta


def test_model_against_the_reference_dead_code():
    """One iteration of the model against the reference's `#if 0` body.  H, Jres and the residual image are exact sums at p = 0 and must be EQUAL; the step may differ
    by the declared departure (f64 solve against Eigen's f32 ldlt): at most 1e-4 of the step's size (largest component) on patches with cond(H) <= 100 -- f32
    epsilon (6e-8) x condition number x the handful of operations of a 2 x 2 solve, with a decade of margin."""
    img, disp, K, uv = _random_records(7, 600)
    n_cmp = 0
    worst = 0.0
    for r in range(len(K)):
        u, v = int(uv[r, 0]), int(uv[r, 1])
        if not (6 <= u < 58 and 6 <= v < 42):
            continue
        gx, gy = M.gradients(K[r])
        H00, H01, H11, det = M.normal_matrix(gx, gy)
        H, Jres, diff, delta = _dead_code(K[r], img, u, v)
        assert H.dtype == f32 and (float(H[0, 0]), float(H[0, 1]), float(H[1, 0]), float(H[1, 1])) == (H00, H01, H01, H11)
        if not det > 0:
            continue
        dx, dy, d, b0, b1 = M.gn_step(K[r], gx, gy, H00, H01, H11, det, img, u, v, f32(0), f32(0))
        assert d.tobytes() == diff.tobytes() and (float(Jres[0]), float(Jres[1])) == (b0, b1)
        if np.linalg.cond(np.array([[H00, H01], [H01, H11]])) <= 100:
            n_cmp += 1
            size = max(abs(float(dx)), abs(float(dy)))
            err = max(abs(float(delta[0]) - float(dx)), abs(float(delta[1]) - float(dy))) / size
            worst = max(worst, err)
            assert err <= 1e-4, (r, delta, dx, dy)
    print("steps compared", n_cmp, "worst relative difference %.2e" % worst)
    assert n_cmp >= 200


def subpixel_accuracy(seed=2024, n=200):
    """The model at 8 iterations on a band-limited texture (synth.band_noise at 1024 texels, 4 octaves: its finest grid is 16 texels = 8 pixels at the 2 texels per
    pixel every level is rendered with) displaced by known shifts uniform in (-0.5, 0.5)^2.  Per level: (RMS error of the integer positions, RMS error of the REFINED
    records, share of REFINED), errors in pixels of the level."""
    from scavislam_amd import synth
    out = []
    for lvl in range(3):
        rng = np.random.default_rng(seed + lvl)
        tex = synth.band_noise(rng, 1024, 4)

        def sample(x, y):
            x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
            fx, fy = x - x0, y - y0
            return (tex[y0, x0] * (1 - fx) + tex[y0, x0 + 1] * fx) * (1 - fy) + (tex[y0 + 1, x0] * (1 - fx) + tex[y0 + 1, x0 + 1] * fx) * fy
        e_int, e_ref, n_ref = [], [], 0
        gy, gx = np.mgrid[0:24, 0:24].astype(np.float64)
        for _ in range(n):
            ox, oy = rng.uniform(40, 900, 2)
            sh = rng.uniform(-0.5, 0.5, 2)
            key = np.clip(np.rint(sample(ox + 2 * gx, oy + 2 * gy)), 0, 255).astype(np.uint8)                            # key(x, y) = tex(o + 2 (x, y))
            cur = np.clip(np.rint(sample(ox + 2 * (gx - sh[0]), oy + 2 * (gy - sh[1]))), 0, 255).astype(np.uint8)    # cur(x, y) = key((x, y) - shift)
            u = v = 12
            K = key[v - 5:v + 5, u - 5:u + 5]
            disp = np.full((24 << lvl, 24 << lvl), 3.0, np.float32)
            st, obs, info = M.refine_patch(K, cur, disp, lvl, u, v, np.zeros(3), 8, 1.5, 0.03)
            e_int.append(sh)
            if info["state"] == M.REFINED:
                n_ref += 1
                e_ref.append((float(info["dx"]) - sh[0], float(info["dy"]) - sh[1]))
                assert obs[0] == float(f32(u) + info["dx"]) * (1 << lvl)
        rms = lambda e: float(np.sqrt((np.asarray(e) ** 2).sum(1).mean()))      # noqa: E731
        out.append((rms(e_int), rms(e_ref), n_ref / n))
    return out


def test_model_finds_subpixel_positions():
    """The refinement halves the position error at least, on every level, and refines at least 90 % of the records."""
    for lvl, (e_int, e_ref, share) in enumerate(subpixel_accuracy()):
        print("level %d: RMS error integer %.4f px, refined %.4f px, REFINED %.1f %%" % (lvl, e_int, e_ref, 100 * share))
        assert e_ref <= 0.5 * e_int, (lvl, e_int, e_ref)
        assert share >= 0.9, (lvl, share)
