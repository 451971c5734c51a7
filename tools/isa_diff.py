"""Is the gfx950 device code of some csrc/*.hip files the same at two revisions?  (No GPU needed.)

    python tools/isa_diff.py --base HEAD~1 [--out profiles/NAME.txt] [FILE.hip ...]

Each file is compiled at the base revision (sources and headers from `git archive`) and in the working tree with build.py's flags plus
`--cuda-device-only -S`, once with the default flag set and once with RECMV_NO_PACKED_F32=1's.  Comment lines and assembler
directives are dropped (labels and the .amdhsa_* kernel descriptors stay; block labels without the index of their function in the
file), and so is the __hip_cuid_* symbol, a hash of the source text.  A line per file and flag set: `identical`, or the functions whose text differs.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("recmv_build", ROOT / "rec-mv_amd" / "build.py")
recmv_build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recmv_build)

DEFAULT_FILES = ["elementwise.hip", "linear_bwd.hip", "mlp_chain.hip", "mlp_jet.hip", "mlp_rows.hip", "gemm_f32.hip", "gemm_tn.hip",
                 "marching_cubes.hip"]
FLAG_SETS = {"default": [], "RECMV_NO_PACKED_F32=1": recmv_build.NO_PACKED_F32}


def device_asm(tree: Path, name: str, extra: list) -> dict:
    """{function or '' for what stands outside one: [lines]} of the normalised device assembly."""
    flags = [f for f in recmv_build.COMMON_FLAGS if not f.startswith("-I")] + [f"-I{tree / 'include'}"]
    cmd = [recmv_build.hipcc(), *flags, *extra, "--cuda-device-only", "-S", str(tree / "rec-mv_amd" / "csrc" / name), "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {name} in {tree}:\n{r.stderr}")
    out, cur = {"": []}, ""
    for line in r.stdout.splitlines():
        s = line.split(";", 1)[0].strip()
        if not s or "__hip_cuid_" in s:
            continue
        if s.startswith(".") and not s.endswith(":") and not s.startswith(".amdhsa_"):
            continue
        s = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", s)      # local labels carry the function's index in the file: it moves when a kernel is added
        m = re.fullmatch(r"([A-Za-z_][\w$.]*):", s)
        if m:
            cur = m.group(1)
            out.setdefault(cur, [])
        out[cur].append(s)
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--out")
    ap.add_argument("files", nargs="*", default=DEFAULT_FILES)
    a = ap.parse_args()
    base_rev = subprocess.check_output(["git", "rev-parse", "--short", a.base], cwd=ROOT, text=True).strip()
    lines = [f"device assembly (gfx950) of the working tree against {base_rev}; tools/isa_diff.py"]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", a.base, "rec-mv_amd/csrc", "include"], cwd=ROOT, capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        jobs = [(f, k) for k in FLAG_SETS for f in a.files]
        with cf.ThreadPoolExecutor(max_workers=8) as ex:
            res = list(ex.map(lambda j: (device_asm(Path(tmp), j[0], FLAG_SETS[j[1]]), device_asm(ROOT, j[0], FLAG_SETS[j[1]])), jobs))
    bad = 0
    for (f, k), (old, new) in zip(jobs, res):
        diff = sorted(n or "(outside a function)" for n in set(old) | set(new) if old.get(n) != new.get(n))
        bad += bool(diff)
        n_lines = sum(len(v) for v in new.values())
        lines.append(f"{f:22s} {k:22s} {n_lines:7d} lines  " + ("identical" if not diff else "DIFFERS: " + " ".join(diff)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        Path(a.out).write_text(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
