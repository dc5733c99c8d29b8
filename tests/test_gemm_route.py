"""Which GEMM kernel runs for which call, pinned on the CPU.  vidi_amd/csrc/gemm_route.h is the one place that decides (pure integer logic);
tools/gemm_route_dump.hip prints its decision per call from a host-only build.  tests/golden/gemm_routes.json holds the calls — every GEMM
the two engines make at the real dimensions on both sides of the 192-tile threshold, every entry point x tile_cfg x K in {64 .. 256} x
widths on both sides of the 288-wide geometry, every epilogue combination on the automatic route, each environment switch at its other
value, refused calls and calls wrong in two ways — with the lines recorded from the launchers of the commit BEFORE the router existed."""
import itertools
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    return "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc")


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """the dump tool, built once (host-only): lines of cases in, lines of routes out"""
    hipcc = _hipcc()
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_dump")
    r = subprocess.run([hipcc, "--cuda-host-only", "-std=c++17", os.path.join(ROOT, "tools", "gemm_route_dump.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(cases):
        r = subprocess.run([exe], input="".join(c + "\n" for c in cases), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        got = r.stdout.splitlines()
        assert len(got) == len(cases)
        return got
    return run


def expand(group):
    """'kind k=a,b j=c' -> the cases of the cross product of the listed values, first key slowest"""
    kind, *toks = group.split()
    keys, vals = zip(*(t.split("=") for t in toks))
    return [kind + "".join(f" {k}={v}" for k, v in zip(keys, combo)) for combo in itertools.product(*(v.split(",") for v in vals))]


@pytest.fixture(scope="module")
def routes(dump):
    with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as f:
        fx = json.load(f)
    cases, want = [], []
    for group, answers in fx["groups"]:
        cases += expand(group)
        want += [fx["routes"][int(a)] for a in answers.split()]
    assert len(cases) == len(want) > 4000
    return list(zip(cases, want, dump(cases)))


def test_routes_match_the_recorded_launches(routes):
    bad = [(c, want, got) for c, want, got in routes if want != got]
    assert not bad, f"{len(bad)} of {len(routes)} routes differ, e.g. {bad[:5]}"


def test_fixture_reaches_every_instantiation(routes):
    """the fixture is only a pin if it launches everything the table in gemm_route.h lists: each enumerator's name must be some case's answer"""
    src = open(os.path.join(ROOT, "vidi_amd", "csrc", "gemm_route.h")).read()
    rows = re.findall(r"^\s+X\((GK_\w+),", src, re.M)
    assert len(rows) == 5 + 11 + 6 + 4 + 3, rows
    seen = {want.split(" ")[0] for _, want, _ in routes if not want.startswith("err")}
    assert len(seen) == len(rows) + 1, sorted(seen)            # + the register-staged kernel
    assert {w for _, w, _ in routes if w.startswith("err")} == {"err -1", "err -2", "err -3", "err -4"}


def test_statistics_calls_are_validated_at_every_width(dump):
    """the one place where the router deliberately departs from the recorded launchers: a vidi_gemm_res_stats call at a width of the 288-wide
    geometry used to reach that kernel without the stride / pointer checks every other call gets (the same call at N = 1 280 was refused)"""
    assert dump(["res_stats M=20000 N=1152 K=1152 ldx=1156", "res_stats M=20000 N=1152 K=1152 ldw=1156 cfg=5", "res_stats M=20000 N=1280 K=1152 ldx=1156"]) == ["err -3"] * 3
