"""CPU tier: the walk of the fixed-point scatter kernels (peleanalysis_amd/csrc/pa_celltiles.h: jpdf, conditionalMean, integral, rmsVel).
tests/celltiles_host.hip is a stand-alone program around the header; it counts the tile table with the function the library uploads
from, decodes every (tile, thread) and reports how often each valid cell of each box was visited.  Built twice -- plain, and with the
address and undefined-behaviour sanitizers on the host code -- and for every (aax, march, kt) the library launches, on the smallest
shapes that can go wrong: every cell exactly once, nothing outside a box, the same box and march bounds in every thread of a tile."""
import os
import shutil
import subprocess

import pytest

import fixed_sums_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "peleanalysis_amd", "csrc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
WALKS = [(aax, march, kt) for aax, march in ((1, 2), (2, 1)) for kt in (16, 64, 128)]  # pa_integral_add_level; the statistics: (1, 2, 16)


def _hipcc():
    cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cc if os.path.exists(cc) else shutil.which("hipcc")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("celltiles") / ("celltiles_host_" + request.param))
    cmd = [cc, "--offload-arch=gfx950", "-O1", "-g", "-I", CSRC, os.path.join(HERE, "celltiles_host.hip"), "-o", exe] + (SAN if request.param == "sanitized" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def box(aax, march, lo, nx, na, nm):
    """a box with corner lo, nx cells along x, na along aax and nm along march"""
    n = [0, 0, 0]
    n[0], n[aax], n[march] = nx, na, nm
    return [*lo, *(lo[d] + n[d] - 1 for d in range(3))]


def levels(aax, march, kt):
    """-> list of (name, boxes)"""
    out = [("one cell", [[3, -2, 7, 3, -2, 7]]),
           ("odd: boxes 12 and 5 cells wide", [[int(v) for v in b] for b in C.hierarchies()["odd"].levels[0].boxes]),
           ("64 x 8 x 8", [[0, 0, 0, 63, 7, 7]]),
           ("a plane of exactly 256 cells", [box(aax, march, (0, 0, 0), 16, 16, 3)]),
           ("a plane of exactly 257 cells", [box(aax, march, (-5, 4, 9), 257, 1, 3)])]
    for nm in (kt - 1, kt, kt + 1):
        out.append((f"march extent {nm}", [box(aax, march, (1, 2, 3), 5, 3, nm)]))
    # boxes of different extents side by side: 1, 4, 9, 1, 6, 1, 1, 4 tiles, so the binary search in cum meets unequal steps
    mixed, x = [], -40
    for nx, na, nm in ((1, 1, 1), (20, 13, kt + 1), (64, 9, 2 * kt + 1), (5, 3, kt - 1), (257, 1, 3 * kt), (12, 8, 1), (16, 16, kt), (33, 8, kt + 2)):
        mixed.append(box(aax, march, (x, -3, 11), nx, na, nm))
        x += nx
    out.append(("boxes of different extents", mixed))
    return out


def ntiles(aax, march, kt, b):
    n = [b[3 + d] - b[d] + 1 for d in range(3)]
    return -(-n[0] * n[aax] // 256) * -(-n[march] // kt)


@pytest.mark.parametrize("aax,march,kt", WALKS)
def test_every_cell_of_every_box_exactly_once(program, aax, march, kt):
    cases = levels(aax, march, kt)
    text = "".join(f"{aax} {march} {kt} {len(bx)}\n" + "".join(" ".join(map(str, b)) + "\n" for b in bx) for _, bx in cases)
    r = subprocess.run([program], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stderr[-4000:]}"
    lines = iter(r.stdout.splitlines())
    for name, bx in cases:
        what = f"(aax, march, kt) = ({aax}, {march}, {kt}), {name}"
        head = next(lines).split()
        assert head[0] == "T", what
        nt, outside, ragged = (int(v) for v in head[1:])
        assert nt == sum(ntiles(aax, march, kt, b) for b in bx), f"{what}: {nt} tiles"
        assert outside == 0, f"{what}: {outside} visits outside the box"
        assert ragged == 0, f"{what}: {ragged} tiles whose threads disagree on the box or the march bounds"
        for ib, b in enumerate(bx):
            seen = next(lines)
            ncell = (b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1)
            assert len(seen) == ncell, f"{what}, box {ib}"
            assert seen == "1" * ncell, f"{what}, box {ib} {b}: {seen.count('0')} cells never visited, {ncell - seen.count('0') - seen.count('1')} more than once"
    assert next(lines, None) is None
