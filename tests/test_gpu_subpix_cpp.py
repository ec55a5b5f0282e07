"""tests/cpp/subpix_smoke.cpp: GuidedMatcher::refineSubpixel and StereoFrontend::setSubpixelAccuracy of include/scavislam_hip.hpp, compiled with
g++ -std=c++11 -Wall -Werror as the other smoke programs are, run on the GPU.  The program itself holds the stateless call against the step with the option on;
the records and svs_subpix_info it writes are held here against the Python binding's on the same frame and candidates, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 320, 240


def _frame():
    """the program's frame: a linear congruential generator, one draw per pixel"""
    img, disp = np.zeros(W * H, np.uint8), np.zeros(W * H, np.float32)
    s = 12345
    for i in range(W * H):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        img[i], disp[i] = s >> 24, 4.0 + ((s >> 12) & 7)
    return img.reshape(H, W), disp.reshape(H, W)


def test_cpp_adaptor_against_the_python_binding(gpu_ctx, tmp_path):
    from scavislam_amd.ctypes_types import CANDIDATE_DTYPE, MATCH_RESULT_DTYPE, SUBPIX_INFO_DTYPE, SUBPIX_REFINED
    from scavislam_amd.frontend import StereoFrontend
    exe, dump = tmp_path / "subpix_smoke", tmp_path / "records.bin"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "subpix_smoke.cpp"),
                           "-o", str(exe), "-L", libdir, "-lscavislam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(dump)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    print(out)
    tok = [l for l in out.splitlines() if l.startswith("SUBPIX ")]
    assert tok and tok[0].split()[1] == "ok", out
    n, matched, refined = (int(x) for x in tok[0].split()[2:5])
    assert n > 100 and matched >= 40 and refined >= 1, tok
    raw = dump.read_bytes()
    arrays, off = [], 0
    for dt in (CANDIDATE_DTYPE, MATCH_RESULT_DTYPE, SUBPIX_INFO_DTYPE):
        k = int(np.frombuffer(raw, np.int32, 1, off)[0])
        arrays.append(np.frombuffer(raw, dt, k, off + 4))
        off += 4 + k * dt.itemsize
    pts, m_cpp, info_cpp = arrays
    assert off == len(raw) and len(pts) == len(m_cpp) == len(info_cpp) == n
    ctx, _ = gpu_ctx
    img, disp = _frame()
    cam = dict(f=285.0, cx=160.0, cy=120.0, b=0.075, w=W, h=H)
    I34 = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
    fe = StereoFrontend(ctx, cam, max_points=1024, max_keyframes=2)
    fe.processFirstFrame(img, disp=disp)
    fe.keepKeyframe(0, I34)
    fe.setCandidates(pts, len(pts))
    fe.setSubpixel()
    _, m, _ = fe.processFrame(img, I34, I34, disp=disp)
    info = fe.subpixelInfo(0)
    fe.close()
    assert m.tobytes() == m_cpp.tobytes() and info.tobytes() == info_cpp.tobytes()
    assert int((info["state"] == SUBPIX_REFINED).sum()) == refined
