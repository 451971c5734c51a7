"""The route planner of csrc/gemm_route.h without a GPU: tools/gemm_route_host_check (the header alone, built with ROCm's clang++ under
the address and undefined-behaviour sanitizers) plans every case of tests/gemm_route_cases.py under the three switch settings, and the
plans are compared with what the library did on an MI355X at the commit before the planner existed (tests/golden/gemm_routes.json,
tests/golden/make_golden_gemm_routes.py): the profile slot that received the launch and the route names it logged.
"""
import json
import subprocess
import sys
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
REPO = HERE.parent
sys.path[:0] = [str(HERE)]
import gemm_route_cases as GC  # noqa: E402
import host_check  # noqa: E402

BM = BN = 128
BK = 32
N_CU = 256


@pytest.fixture(scope="module")
def census():
    return json.loads((HERE / "golden" / "gemm_routes.json").read_text())["settings"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{setting: {case name: the fields the program printed}}"""
    check = host_check.build("gemm_route", tmp_path_factory.mktemp("gemm_route_host_check"))
    out = {}
    for setting in GC.SETTINGS:
        text = "".join(GC.host_line(c, setting) + "\n" for c in GC.CASES)
        r = subprocess.run([str(check)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        rows = [ln.split("\t") for ln in r.stdout.splitlines()]
        out[setting] = {row[0]: row[1:] for row in rows}
    return out


def test_every_case_is_in_the_census_and_planned(census, plans):
    names = sorted(c["name"] for c in GC.CASES)
    assert sorted(GC.SETTINGS) == sorted(census) == sorted(plans)
    for setting in GC.SETTINGS:
        assert sorted(census[setting]) == names and sorted(plans[setting]) == names, setting


@pytest.mark.parametrize("setting", sorted(GC.SETTINGS))
def test_slot_and_logged_route_equal_the_census(census, plans, setting):
    for c in GC.CASES:
        want, got = census[setting][c["name"]], plans[setting][c["name"]]
        print(setting, c["name"], got)
        assert int(got[1]) == want["slot"], (setting, c["name"], got, want)
        assert (got[2], got[3]) == (want["route"], want["before"]), (setting, c["name"], got, want)


def test_thin_n_order_is_that_of_the_mfma_route(plans):
    """`halves` (the summation order of the 64 x 32 kernel) exactly where the plan without the skinny routes is that kernel; the two
    sides of the 640-row-tile boundary take different orders."""
    thin = [c["name"] for c in GC.CASES if plans["default"][c["name"]][0] == "ThinN"]
    assert {"nt_thin_n4_M40896", "nt_thin_n4_M40897", "nt_thin_n1", "nt_thin_n3", "nt_thin_n4", "mulgrad_thin_n3", "seg_thin_n3",
            "mulgrad_seg_thin_n3"} == set(thin)
    for name in thin:
        kernel, slot, route, parent, halves, mfma = plans["default"][name]
        assert (halves == "1") == (mfma == "Narrow"), (name, halves, mfma)
        assert plans["skinny0"][name][0] == mfma            # ... and that plan is what RECMV_GEMM_SKINNY=0 launches
    assert plans["default"]["nt_thin_n4_M40896"][4] == "1" and plans["default"]["nt_thin_n4_M40897"][4] == "0"
    assert "actgrad_n3" not in thin


def tn_splits(M, N, K):
    """recmv_gemm_tn_workspace_bytes / (M N 4): ~4 workgroups per CU over the 128 x 128 output tiles, at least 4 K-tiles of 32 rows per
    split, at most 128 splits."""
    tiles = -(-M // BM) * -(-N // BN)
    return max(1, min(-(-N_CU * 4 // tiles), -(-K // (BK * 4)), 128))


def test_tn_splits_and_split_lengths(plans):
    tn = [c for c in GC.CASES if c["entry"] == "tn"]
    assert len(tn) == 7
    for setting in GC.SETTINGS:
        for c in tn:
            kernel, slot, route, parent, swap, splits, kchunk = plans[setting][c["name"]]
            M, N, K = c["M"], c["N"], c["K"]
            assert int(splits) * M * N * 4 == tn_splits(M, N, K) * M * N * 4, (setting, c["name"])
            # split lengths: K / splits rounded up to the K-tile of the MFMA kernel that has (or had) the launch: 16 rows for the aligned
            # high-occupancy kernel, 32 for the others (the thin and the SCAL kernels keep the length of the kernel they replace)
            tile = 16 if kernel == "Occ" or (kernel == "Thin" and c["name"] == "tn_4x512") else 32
            assert int(kchunk) == -(-(-(-K // int(splits))) // tile) * tile, (setting, c["name"], kernel, kchunk)
