"""The software pipeline of the fused sweeps, read off the device assembly (host tier; compiles pa_fused_sweep.hip to gfx950
assembly only, about a minute).

A storing step of an output row issues 8 stores and 1 load and takes the plane it requested three steps earlier, so the
marching loop (three steps per trip: 24 `global_store_dwordx2`) should wait with the operations of the two steps before still in
flight -- the same `s_waitcnt vmcnt(N)` in each of its three steps.  The compiler derives N per step from everything that can be
in flight on ANY edge into the loop: a request left pending on the entry edge once cost the exact-normal variants two of their
three planes of latency cover in one step out of three (waits 18, 9, none) without changing a result.  This test holds every
`k_gradcurv_march3*` kernel to "all waits of a 24-store loop are equal".  It reads wait counts and store counts, nothing else."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "peleanalysis_amd", "csrc")


def _kernels(path):
    """{symbol: lines} of the kernels whose name holds k_gradcurv_march3"""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w*k_gradcurv_march3\w*):", line)
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None:
                if line.startswith(".Lfunc_end"):
                    cur = None
                else:
                    cur.append(line)
    return out


def _loops(lines):
    """(first, last) line of every backward branch's range"""
    label = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label[m.group(1)] = i
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and label.get(m.group(1), i) < i:
            yield label[m.group(1)], i


def test_marching_loops_wait_evenly(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc) or shutil.which(hipcc), f"no hipcc at {hipcc}"
    asm = str(tmp_path / "pa_fused_sweep.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                           os.path.join(CSRC, "pa_fused_sweep.hip"), "-o", asm], stderr=subprocess.DEVNULL)
    kernels = _kernels(asm)
    assert len(kernels) >= 20, sorted(kernels)
    checked, uneven = {}, []
    for name, lines in sorted(kernels.items()):
        for a, b in _loops(lines):
            body = lines[a:b + 1]
            if sum("global_store_dwordx2" in l for l in body) != 24:
                continue
            waits = [int(m.group(1)) for l in body for m in [re.search(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", l)] if m]
            checked[name] = checked.get(name, 0) + 1
            print(f"{name}: lines {a}-{b}: vmcnt {waits}")
            if len(waits) < 3 or len(set(waits)) != 1:
                uneven.append((name, waits))
    # the headline kernel (13-row tiles, no clip, 8 outputs) and the narrow-box all-levels kernel are among the kernels checked
    assert any(n.startswith("_Z24k_gradcurv_march3_levelsILi13ELb0ELi0E") for n in checked), sorted(checked)
    assert any(n.startswith("_Z25k_gradcurv_march3n_levelsILi8ELb0ELb0E") for n in checked), sorted(checked)
    assert len(checked) >= 20, sorted(checked)
    assert not uneven, "marching loops whose steps wait at different depths: " + "; ".join(f"{n}: {w}" for n, w in uneven)
