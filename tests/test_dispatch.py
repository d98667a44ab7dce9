"""The width dispatch of the SELL-family launchers (vexcl_amd/csrc/dispatch.hpp) maps a run-time ELL width to a template argument.
A wrong mapping is silent on the device (the pair kernels take the width at compile time only: a wrong one is a wrong slice stride),
and the halo and march forms cannot cheaply be driven at every width there, so the mapping is pinned on the host: a stand-alone
program (tests/cpp/dispatch_widths.cpp), plain g++, no HIP and no library code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_width_dispatch_maps_every_width_once(tmp_path):
    exe = str(tmp_path / "dispatch_widths")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + ROOT, os.path.join(ROOT, "tests", "cpp", "dispatch_widths.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "0 failures", out.stdout
