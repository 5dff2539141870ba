"""The frame view's layout (kernels.h FrameArgs), without a GPU.

The kernels fetch the view in aligned blocks, so the offsets are part of the
contract between make_frame_view (host) and view_block (device):

1. kernels.h's static_asserts on every offset hold in the host pass and in the
   gfx950 device pass of a translation unit that includes it;
2. a view built by the library's make_frame_view, read back field by field at
   those offsets, equals what was set (tests/api/view_layout_check.hip, linked
   against the built library; nothing in it touches a device).
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "api", "view_layout_check.hip")
FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cairo_amd", "csrc")]


def test_layout_asserts_compile_for_host_and_device():
    for side in ("--cuda-host-only", "--cuda-device-only"):
        r = subprocess.run([HIPCC, *FLAGS, side, "-fsyntax-only", SRC], capture_output=True, text=True)
        assert r.returncode == 0, f"{side}:\n{r.stderr}"


def test_host_built_view_reads_back(cairo, tmp_path):
    exe = str(tmp_path / "view_layout_check")
    libdir = os.path.dirname(cairo.LIB_PATH)
    r = subprocess.run([HIPCC, *FLAGS, SRC, "-o", exe, "-L", libdir, "-lcairo_amd", f"-Wl,-rpath,{libdir}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: ") or "\nok: " in r.stdout
    assert "512 bytes" in r.stdout and " 0 mismatches" in r.stdout
