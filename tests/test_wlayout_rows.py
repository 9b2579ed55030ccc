"""The storage-row permutation of the window layout (metmhn_amd/csrc/wlayout.h) on the host.

tests/host/wlayout_check.hip is a stand-alone program (own main, no GPU runtime call): wrho is a bijection that wrho_inv
inverts, every (wave, lane-level) group is one contiguous run, wpos_marg agrees with wpos_nat on both of its branches, and
the lines a block's steps request - counted once per (lane-level, wave-level) class that has a row in them - stay below
the 304 lines of 128 bytes / 544 of 64 bytes of the order the layout had before.  It is compiled here with the host
sanitizers (address, undefined behaviour) into pytest's temporary directory and run as a child process; the sanitizers
stay in that binary.  No GPU is needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wlayout_check.hip")


def test_window_rows_permutation_and_line_model(tmp_path):
    exe = str(tmp_path / "wlayout_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")           # (the compiler of metmhn_amd/_lib.py: build)
    cmd = [hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Wno-comment", "-Xarch_host", "-fsanitize=address,undefined",
           "-I", os.path.join(ROOT, "metmhn_amd", "csrc"), "-o", exe, SRC]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, "hipcc failed:\n" + res.stderr[-4000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(res.stdout)
    print(res.stderr[-4000:])
    assert res.returncode == 0, "wlayout_check reported a violation (or a sanitizer did):\n" + res.stdout[-2000:] + res.stderr[-4000:]
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr
    fig = {m.group(1): int(m.group(2)) for m in re.finditer(r"^(\w[\w ]*?) (\d+)$", res.stdout, re.M)}
    assert fig["groups"] == 16 * 7 and fig["marginal states"] > 0
    # a block is 256 lines of 128 bytes; before: 304 lines, 544 half-lines
    assert 256 <= fig["lines128"] < 304, fig
    assert 512 <= fig["lines64"] < 544, fig
