"""Byte counts of the MLP workspaces as librecmv_hip.so computes them: tests/test_mlp_desc_cpu.py's layout table (the chain's
workspace with and without kept activations, the jet's, the row-tile kernels' and their packed weights) for three nets of
tests/mlp_reference.py at four row counts.  Host functions only: no GPU is needed.

  mlp_workspace_bytes.json   {"commit": the commit of the library that was measured, "bytes": {net: {P: {function: bytes}}}}

A change that must keep the layouts takes its expectations from the commit before it: build that commit's library and run this with
RECMV_LIB_PATH pointing at it.

    python tests/golden/make_golden_mlp_workspace_bytes.py [COMMIT]      # COMMIT: where the tree is no git checkout
"""
import json
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path[:0] = [str(HERE.parent), str(REPO / "rec-mv_amd"), str(REPO)]
import test_mlp_desc_cpu as T  # noqa: E402


def main():
    commit = sys.argv[1] if sys.argv[1:] else subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True,
                                                             text=True).stdout.strip()
    from recmv import _lib
    table = T.layout_table(_lib.lib())
    (HERE / "mlp_workspace_bytes.json").write_text(json.dumps({"commit": commit, "bytes": table}, indent=1, sort_keys=True) + "\n")
    print(json.dumps(table["sdf"]["33"]))


if __name__ == "__main__":
    main()
