"""The census of the GEMM routes: which profile slot, which logged route and which bits every case of tests/gemm_route_cases.py gets
from librecmv_hip.so on an MI355X, under three switch settings (default, RECMV_GEMM_SKINNY=0, RECMV_GEMM_OCC=0).

  gemm_routes.json
    commit     the commit of the library that was measured (the expectations of a change to the host-side route code come from the
               commit before it: run this there, before the change is applied)
    settings   {setting: {case name: {"slot": int, "route": str, "before": str, "digest": 16 hex digits}}}
               slot    the one of the 14 profile slots that received the case's product launch (recmv_profile_begin(0) / _end(.., 14))
               route / before   the two names of the case's `[recmv shapes]` line (RECMV_GEMM_SHAPES=1), empty if it logged none
               digest  gemm_route_cases.digest of the output, computed on the device

One fresh child process per setting, one after the other, each under a time limit; this process never opens the GPU and reads the
`[recmv shapes]` lines from the child's stderr (the child announces every case on stderr before it runs it).

    python tests/golden/make_golden_gemm_routes.py [COMMIT]      # COMMIT: where the tree is no git checkout
"""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path[:0] = [str(HERE.parent), str(REPO / "rec-mv_amd"), str(REPO)]
import gemm_route_cases as GC  # noqa: E402

CHILD_TIMEOUT_S = 240
SHAPES = re.compile(r"^\[recmv shapes\] (\S+) \(before: (.*?)\) M=")


def child():
    import torch
    from recmv import _lib as L
    L.set_gemm_mode(0)
    for c in GC.CASES:
        sys.stderr.write("[case] %s\n" % c["name"])
        sys.stderr.flush()
        slot, out = GC.profiled_slot(c)
        torch.cuda.synchronize()
        print(json.dumps({"name": c["name"], "slot": slot, "digest": GC.digest(out)}), flush=True)


def main():
    commit = sys.argv[1] if sys.argv[1:] else subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=REPO, capture_output=True,
                                                             text=True).stdout.strip()
    settings = {}
    for setting, env in GC.SETTINGS.items():
        full = {k: v for k, v in os.environ.items() if k not in ("RECMV_GEMM_SKINNY", "RECMV_GEMM_OCC")}
        full.update(env, RECMV_GEMM_SHAPES="1")
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, __file__, "child"], env=full,
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("setting %s: child ended with %d\n%s" % (setting, r.returncode, r.stderr[-4000:]))
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                res[d.pop("name")] = dict(d, route="", before="")
        cur = None
        for line in r.stderr.splitlines():
            if line.startswith("[case] "):
                cur = line[7:]
            m = SHAPES.match(line)
            if m:
                assert res[cur]["route"] == "", "two shape lines in case " + cur
                res[cur].update(route=m.group(1), before=m.group(2))
        assert sorted(res) == sorted(c["name"] for c in GC.CASES)
        settings[setting] = res
        print("%s: %d cases" % (setting, len(res)))
    (HERE / "gemm_routes.json").write_text(json.dumps({"commit": commit, "settings": settings}, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    child() if sys.argv[1:] == ["child"] else main()
