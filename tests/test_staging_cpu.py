"""scavislam_amd/csrc/pieces.h, the offset part of the library's staged calls (staging.h; map.hip and frontend.hip lay every block out with it): compiled
for the host alone, without HIP headers, under AddressSanitizer and UBSan as a stand-alone program (tests/cpp/staging_host.cpp, which states what it checks)
and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pieces_host_only_under_sanitizers(tmp_path):
    exe = tmp_path / "staging_host"
    # (the sanitizers' runtimes linked into the program: it runs the same whatever else the environment loads in front of it)
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           os.path.join(ROOT, "tests", "cpp", "staging_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "staging_host ok" in r.stdout
