"""The cohort planner (metmhn_amd/csrc/plan.h) against brute force on the host.

tests/host/plan_check.hip is a stand-alone program (own main, no GPU runtime call) that plans generated cohorts under a
sweep of configurations and checks every work list, offset and layout against a model written out in the program: the
states of every tile are enumerated, and the moves of the model decide which tiles are dead and which tiles a tile of the
cooperative solve has to wait for.  It is compiled here with the host sanitizers (address, undefined behaviour) into
pytest's temporary directory and run as a child process; the sanitizers stay in that binary.  No GPU is needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "plan_check.hip")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # (the compiler of metmhn_amd/_lib.py: build)
    cmd = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-comment", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "metmhn_amd", "csrc"), "-o", exe, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, "hipcc failed:\n" + res.stderr[-4000:]
    return exe


def _run(exe, *args):
    res = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    print(res.stderr[-4000:])
    assert res.returncode == 0, "plan_check reported a violation (or a sanitizer did):\n" + res.stdout[-2000:] + res.stderr[-4000:]
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^count (.*): (-?\d+)$", res.stdout, re.M)}
    checks = {m.group(1).strip(): tuple(int(v) for v in m.group(2, 3, 4))
              for m in re.finditer(r"^check (.*?)\s+plans\s+(\d+)\s+problems\s+(\d+)\s+tiles\s+(\d+)$", res.stdout, re.M)}
    return counts, checks


def test_planner_lists_against_enumeration(plan_check):
    """Every list of every plan of the sweep; the targeted shapes must have been reached."""
    counts, checks = _run(plan_check)
    for name in ("batches", "cooperative lists", "dead tiles", "gradient chunks", "layouts", "level lists", "mapX", "paired", "pcl",
                 "ptiles", "rejections", "routes", "small-space classes", "staged groups", "window chains"):
        assert name in checks and checks[name][0] > 0, name
    for name in ("cooperative lists", "dead tiles", "level lists", "ptiles", "staged groups", "mapX", "gradient chunks"):
        assert checks[name][1] > 0 and checks[name][2] > 0, name
    for name in ("straddling tiles", "straddling tiles live without seeding", "dead tiles", "batches with dealt chains",
                 "dealt chain entries left empty", "window chains of several rows", "rows merged into the 256-thread launch",
                 "batches with a launch of the 1024-thread class", "batches with an empty pcl (nJ > prep_split_max)",
                 "plans with a cut cohort", "cohorts with an evenly spread target", "patients with a single-tumour space beyond a tile",
                 "problems on the window route", "problems on the per-patient route", "problems on the tile route",
                 "cooperative dependencies required by the model"):
        assert counts.get(name, 0) > 0, name


def test_tile_edge_cohorts_of_the_gpu_tests(plan_check, tmp_path):
    """The cohorts of tests/test_gpu_parity.py: test_tile_edge_shapes_on_every_route: their plans hold under the configurations
    that test runs, the pair on bits 11 / 12 is among their tiles, and the n = 12 cohort on three window workgroups deals
    its chains (at n = 8 no class reaches the ten bits of a window shape: that cohort never takes the window route)."""
    from metmhn_amd import synthetic
    for n, window in ((8, False), (12, True)):
        dat = synthetic.tile_edge_cohort(n)
        path = tmp_path / f"cohort{n}.bin"
        dat.tofile(path)
        counts, _ = _run(plan_check, "--cohort", str(path), str(dat.shape[0]), str(n))
        assert counts.get("straddling tiles live without seeding", 0) > 0
        assert counts.get("dead tiles", 0) > 0
        assert counts.get("problems on the per-patient route", 0) > 0 and counts.get("problems on the tile route", 0) > 0
        assert counts.get("batches with an empty pcl (nJ > prep_split_max)", 0) > 0
        assert (counts.get("batches with dealt chains", 0) > 0) == window
        assert (counts.get("problems on the window route", 0) > 0) == window
