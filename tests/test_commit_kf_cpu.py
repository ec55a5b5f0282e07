"""CPU tests of inserting a dropped keyframe from device lists (svs_map_add_keyframe_dev, svs_frontend_commit_keyframe): the NumPy model of the check kernel
(tests/commit_kf_model.py: check_stage) against a literal restatement of what svs_map_add_keyframe decides about the same records on the host, on randomized lists;
the new struct against the header; both entry points declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import commit_kf_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _agree(m, new, track, oldkey, rng):
    got = CM.check_stage(m, new, track, oldkey)
    want = CM.host_restatement(m, new, track, oldkey, rng)
    assert (got["status"], got["phase"], got["index"]) == (want["status"], want["phase"], want["index"]), (got, want)
    assert got["new_pid"].tolist() == [int(np.int32(v)) for v in new[0]] and got["track_gid"].tolist() == [int(np.int32(v)) for v in track[0]]
    if want["status"] == CM.OK:
        assert got["flags"].tolist() == want["flags"]
    return got


def test_the_model_equals_the_host_code_on_random_lists():
    rng = np.random.default_rng(2024)
    seen = {}
    for t in range(1500):
        m, new, track, oldkey = CM.random_case(rng, bad=int(rng.integers(0, 3)) if t % 3 else 0)
        got = _agree(m, new, track, oldkey, rng)
        seen[(got["status"], got["phase"])] = seen.get((got["status"], got["phase"]), 0) + 1
        if got["status"] == CM.OK:
            seen["dup"] = seen.get("dup", 0) + int((got["flags"] == 1).any())
            seen["foreign"] = seen.get("foreign", 0) + int((got["flags"] == 0).any())
    # every outcome was met, often enough to mean something
    for key in ((CM.OK, 0), (CM.INVALID, CM.PHASE_ANCHORS), (CM.INVALID, CM.PHASE_NEW), (CM.CAPACITY, CM.PHASE_NEW), (CM.INVALID, CM.PHASE_TRACK),
                (CM.INVALID, CM.PHASE_OLDKEY), "dup", "foreign"):
        assert seen.get(key, 0) >= 10, (key, seen)


def test_the_model_at_the_cases_the_header_names():
    m = dict(max_pt=100, kf={2, 9}, pt={5, 6, 7}, pairs={(5, 2), (6, 9), (7, 9)})
    lv = lambda n: np.zeros(n, np.int64)

    def run(pid, anchor, gid, oldkey=2, la=None, lf=None, lvl=None):
        new = (np.array(pid, np.int64), np.array(anchor, np.int64), lv(len(pid)) if la is None else np.array(la), lv(len(pid)) if lf is None else np.array(lf))
        track = (np.array(gid, np.int64), lv(len(gid)) if lvl is None else np.array(lvl))
        g = _agree(m, new, track, oldkey, None)
        return g["status"], g["phase"], g["index"], g["flags"].tolist()
    assert run([10, 11], [2, 9], [5, 5, 99, -1, 100, 5, 6]) == (CM.OK, 0, -1, [3, 1, 0, 0, 0, 1, 3])
    assert run([], [], [5]) == (CM.OK, 0, -1, [3])                                   # oldkey enters through a track pair alone
    assert run([], [], [6])[:3] == (CM.INVALID, CM.PHASE_OLDKEY, -1)
    assert run([], [], [])[:3] == (CM.INVALID, CM.PHASE_OLDKEY, -1)
    assert run([10], [2], [])[:3] == (CM.OK, 0, -1)
    assert run([10, 11, 12], [2, 3, 4], [])[:3] == (CM.INVALID, CM.PHASE_ANCHORS, 1)
    assert run([10, 5, -1], [2, 2, 2], [])[:3] == (CM.INVALID, CM.PHASE_NEW, 1)    # the first offender, whatever follows
    assert run([10, 100, -1], [2, 2, 2], [])[:3] == (CM.CAPACITY, CM.PHASE_NEW, 1)
    assert run([10, -1, 100], [2, 2, 2], [])[:3] == (CM.INVALID, CM.PHASE_NEW, 1)
    assert run([10, 11, 10], [2, 2, 2], [])[:3] == (CM.INVALID, CM.PHASE_NEW, 2)   # the later of two equal ids
    assert run([10, 11], [2, 2], [], la=[0, 3])[:3] == (CM.INVALID, CM.PHASE_NEW, 1)
    assert run([10, 11], [2, 2], [], lf=[-1, 0])[:3] == (CM.INVALID, CM.PHASE_NEW, 0)
    assert run([10, 11], [2, 2], [5, 11, 10])[:3] == (CM.INVALID, CM.PHASE_TRACK, 1)
    assert run([10], [2], [101, 5], lvl=[3, 0])[:3] == (CM.INVALID, CM.PHASE_TRACK, 0)   # a bad level also on an entry that names no point
    assert run([10, 3], [9, 2], [5, 10])[:3] == (CM.INVALID, CM.PHASE_TRACK, 1)
    assert run([5], [7], [5])[:3] == (CM.INVALID, CM.PHASE_ANCHORS, 0)               # anchors before everything else


SYMBOLS = ["svs_map_add_keyframe_dev", "svs_frontend_commit_keyframe", "svs_map_get_keyframe"]


def test_header_binding_and_exports_agree(tmp_path):
    from scavislam_amd import capi
    from scavislam_amd.ctypes_types import CommitKeyframeRequest
    from scavislam_amd.frontend import StereoFrontend
    from scavislam_amd.register import ResidentMap
    hdr = open(os.path.join(ROOT, "include", "scavislam_hip.h")).read()
    assert int(re.search(r"#define SVS_API_VERSION (\d+)", hdr).group(1)) == capi.API_VERSION == 9
    lib = capi.load()
    for n in SYMBOLS:
        assert n in capi.EXPORTS and re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
    assert callable(ResidentMap.add_keyframe_dev) and callable(StereoFrontend.commitKeyframe)
    names = [f for f, _ in CommitKeyframeRequest._fields_]
    fields = ["offsetof(svs_commit_keyframe_request,%s)" % f for f in names] + ["sizeof(svs_commit_keyframe_request)"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scavislam_hip.h"\nint main(){' + "".join('printf("%%zu\\n",(size_t)%s);' % f for f in fields) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(CommitKeyframeRequest, f).offset for f in names] + [C.sizeof(CommitKeyframeRequest)] and got[-1] == 72


def test_cpp_adaptor_declares_the_calls(tmp_path):
    """BackendMap::addKeyframe from device lists and StereoFrontend::addNewKeyframeToMap (one-stream and batch front ends: one class) compile with plain g++ -std=c++11"""
    src = tmp_path / "a.cpp"
    src.write_text('#include "scavislam_hip.hpp"\n'
                   "using namespace scavislam_hip;\n"
                   "typedef bool (BackendMap::*addkf_dev_fn)(int, const RegistrationKeyframe &, const RegistrationFrame &, const double *, const svs_map_new_point *, int,\n"
                   "                                  const svs_map_track_point *, int, int, const svs_cam &, BackendMap::AddKeyframeResult *, const std::vector<int32_t> &,\n"
                   "                                  const std::vector<double> &, int);\n"
                   "typedef bool (StereoFrontend::*commit_fn)(BackendMap &, int, int, int, const svs_keyframe_decision &, const float *, int, int, const svs_cam &,\n"
                   "                                     BackendMap::AddKeyframeResult *, const std::vector<int32_t> &, const std::vector<double> &, int, int);\n"
                   "addkf_dev_fn f1 = &BackendMap::addKeyframe; commit_fn f2 = &StereoFrontend::addNewKeyframeToMap;\n"
                   "int main(){ Context c(0); if(!c.ok()){ std::puts(\"nodev\"); return 0; } std::puts(\"dev\"); return f1 && f2 ? 0 : 1; }\n")
    exe = tmp_path / "a"
    libdir = os.path.join(ROOT, "scavislam_amd")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lscavislam_hip",
                           f"-Wl,-rpath,{libdir}"])
    assert subprocess.check_output([str(exe)]).decode().strip() in ("nodev", "dev")
