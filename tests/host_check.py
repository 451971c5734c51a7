"""The host checks of tools/*_host_check, built from one recipe: a kernel source compiled for the CPU and run under the address and
undefined-behaviour sanitizers against plain loops, as a stand-alone program (tools/host_check/README.md).

    python tests/host_check.py <name>|all

builds in a temporary folder, runs and prints the program's output; the tests call run() or build() with their tmp_path.
Nothing is copied: main.cpp is compiled where it lies, and the include path puts the folder with the cut kernels first, the
stand-in tools/host_check/common.h second, so that the kernels' `#include "common.h"` finds the stand-in and every other header the
real file."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "rec-mv_amd" / "csrc"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off"]

# check -> ((csrc .hip, the .inc its main.cpp includes), ...), extra flags.  A check without cuts compiles no kernel and gets
# neither the stand-in nor include/.
CHECKS = {
    "mesh_grid": ((("mesh_grid.hip", "kernels.inc"),), ()),
    "mesh_intersect": ((("mesh_grid.hip", "grid.inc"), ("mesh_intersect.hip", "intersect.inc")), ()),
    "segment_mesh": ((("mesh_grid.hip", "grid.inc"), ("segment_mesh.hip", "segment.inc")), ()),
    "mesh_topology": ((("mesh_topology.hip", "topology.inc"),), ()),
    "mesh_simplify": ((("mesh_simplify.hip", "simplify.inc"),), ()),
    "mesh_repair": ((("point_grid.hip", "point_grid.inc"),), ()),
    "voxelize": ((("mesh_voxelize.hip", "voxelize.inc"),), ()),
    "winding": ((("winding.hip", "winding.inc"),), ()),
    "geodesic": ((("geodesic.hip", "geodesic.inc"),), ()),
    "param": ((("mesh_param.hip", "param.inc"),), ()),
    "gemm_route": ((), ("-Wall", "-Werror")),
}

MARKER = re.compile(r"^using namespace recmv;", re.M)       # the kernels end here; the entry points with their HIP calls follow
PRAGMA = re.compile(r"^#pragma clang fp contract\(off\)", re.M)
# headers whose arithmetic must not contract: a helper defined in front of the pragma would fuse its products on the GPU
UNCONTRACTED = re.compile(r'^#include "(?:mesh_device|mesh_cg|closest_tri|grid_query|tri_tri|seg_tri|solid_angle)\.h"', re.M)


def cut(hip):
    """The text of a kernel source up to its `using namespace recmv;` line."""
    text = hip.read_text()
    marks = MARKER.findall(text)
    if len(marks) != 1:
        raise ValueError("%s: %d lines begin with `using namespace recmv;`, the cut needs exactly one" % (hip, len(marks)))
    head = text[:MARKER.search(text).start()]
    header, pragma = UNCONTRACTED.search(head), PRAGMA.search(head)
    if header and not (pragma and pragma.start() < header.start()):
        raise ValueError("%s: `#pragma clang fp contract(off)` must precede %s" % (hip, header.group(0)))
    return head


def build(name, workdir):
    """Cut the kernels into `workdir`, compile tools/<name>_host_check/main.cpp; the path of the program."""
    if not Path(CLANG).exists():
        import pytest
        pytest.skip("ROCm's clang++ not present")
    cuts, extra = CHECKS[name]
    workdir = Path(workdir)
    for hip, inc in cuts:
        (workdir / inc).write_text(cut(CSRC / hip))
    include = [workdir, REPO / "tools" / "host_check", CSRC, REPO / "include"] if cuts else [CSRC]
    subprocess.run([CLANG, *FLAGS, *extra, *("-I" + str(d) for d in include),
                    str(REPO / "tools" / (name + "_host_check") / "main.cpp"), "-o", str(workdir / "check")], check=True)
    return workdir / "check"


def run(name, workdir):
    return subprocess.run([str(build(name, workdir))], cwd=workdir, stdin=subprocess.DEVNULL, capture_output=True, text=True)


def main(argv):
    if len(argv) != 1 or argv[0] not in (*CHECKS, "all"):
        sys.exit("usage: python tests/host_check.py %s|all" % "|".join(CHECKS))
    if not Path(CLANG).exists():
        sys.exit("ROCm's clang++ not present")
    failed = []
    for name in (CHECKS if argv[0] == "all" else argv):
        with tempfile.TemporaryDirectory() as tmp:
            r = run(name, tmp)
        print("==== %s (exit %d)\n%s%s" % (name, r.returncode, r.stdout, r.stderr), flush=True)
        failed += [name] * (r.returncode != 0)
    sys.exit("failed: " + " ".join(failed) if failed else 0)


if __name__ == "__main__":
    main(sys.argv[1:])
