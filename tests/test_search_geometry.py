"""The intra search's candidate geometry and packed source sum, without a GPU.

The row coder derives a lane group's candidate from per-lane unit offsets and
the replay reads the coordinates its group stored (cairo_amd/csrc/
search_geometry.h, host and device).  tests/api/search_geometry_check.hip, a
host program, sweeps

1. every stage 0..4, both halves, every group 0..15 and every replay lane
   0..31 over states around every macroblock of a 160x64 frame, so that
   candidates fall left of, above, right of and below the frame and inside the
   not-yet-coded region (it fails if one of these was not reached): candidate,
   slot validity and replayed coordinates must equal the search's closed form,
   restated in the program;
2. all 65 536 int16 values: the unsigned distance of the biased value from the
   bias, which v_sad_u16 adds up, equals abs().
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "tests", "api", "search_geometry_check.hip")
FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "cairo_amd", "csrc")]


def _run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_geometry") / "search_geometry_check")
    r = subprocess.run([HIPCC, *FLAGS, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    return r


_result = None


def _checked(tmp_path_factory):
    global _result
    if _result is None:
        _result = _run(tmp_path_factory)
    return _result


def test_header_compiles_for_host_and_device():
    for side in ("--cuda-host-only", "--cuda-device-only"):
        r = subprocess.run([HIPCC, *FLAGS, side, "-fsyntax-only", SRC], capture_output=True, text=True)
        assert r.returncode == 0, f"{side}:\n{r.stderr}"


def test_geometry_equals_the_closed_form(tmp_path_factory):
    r = _checked(tmp_path_factory)
    m = re.search(r"geometry: (\d+) checks, (\d+) mismatches; candidates left (\d+) above (\d+) right (\d+) "
                  r"below (\d+) of the frame, (\d+) not yet coded, (\d+) valid", r.stdout)
    assert m, r.stdout + r.stderr
    checks, bad, *regions = map(int, m.groups())
    assert bad == 0, r.stdout
    assert checks > 100000 and all(n > 0 for n in regions), r.stdout
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stdout + r.stderr


def test_biased_absolute_difference_is_abs(tmp_path_factory):
    r = _checked(tmp_path_factory)
    assert "source sum: 65536 values, 0 mismatches" in r.stdout, r.stdout + r.stderr
