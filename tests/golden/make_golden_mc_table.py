"""The marching-cubes triangle table of the reference (`a2iTriangleConnectionTable[256][16]` of MCGpu/CudaKernels.cu), read from
the reference tree -> tests/golden/mc_triangle_table.json (256 rows of 16 edge indices, -1 = end of list);
tests/test_mc_oracle.py decodes the packed tables of oracle/ and rec-mv_amd/csrc/ against it.

    python tests/golden/make_golden_mc_table.py /path/to/reference
"""
import json
import re
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent

if __name__ == "__main__":
    text = (Path(sys.argv[1]) / "MCGpu" / "CudaKernels.cu").read_text()
    m = re.search(r"a2iTriangleConnectionTable\[256\]\[16\]\s*=\s*\{(.*?)\};", text, re.S)
    tri = [int(t) for t in re.findall(r"-?\d+", m.group(1))]
    assert len(tri) == 256 * 16, len(tri)
    rows = [tri[16 * i:16 * i + 16] for i in range(256)]
    (HERE / "mc_triangle_table.json").write_text("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("256 cases,", sum(v >= 0 for v in tri) // 3, "triangles")
