"""bench.py --dump-outputs: the last timed step's outputs at a fixed, seeded sample of cells, so that two builds can be compared
output for output.

* CPU tier: dump_outputs on host tensors whose values encode (cell, component, level) -- every sampled cell is read from the right
  place of the swept tiling, the file's own tiling and the internal one dump the same cells in the same order, the ranks of a
  sharded run dump the sample between them, and the dump stays inside its size budget.
* GPU tier: a plain bench run writes the dump (and nothing of --full into its line), bit for bit the CPU oracle's outputs on
  the same inputs."""
import importlib.util
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch  # noqa: F401  -- before the library: torch's HIP runtime must be the first one the process loads (conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sp = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(m)
    return m


def _encoded_dump(bench, tmp, Hfile, H, owners, rank, nslot):
    from peleanalysis_amd.hierarchy import mf_layout
    dls, touts = [], []
    for l, lv in enumerate(H.levels):
        bx = lv.boxes if owners is None else lv.boxes[np.asarray(owners[l]) == rank]
        dls.append(types.SimpleNamespace(level=types.SimpleNamespace(boxes=bx)))
        off, cs, tot = mf_layout(bx, 8 * nslot, 0)
        t = np.full(max(tot, 1), np.nan)
        for q in range(len(bx)):
            lo, hi = bx[q, :3].astype(np.int64), bx[q, 3:].astype(np.int64)
            k, j, i = np.meshgrid(*(np.arange(lo[d], hi[d] + 1) for d in (2, 1, 0)), indexing="ij")
            n = int(np.prod(hi - lo + 1))
            for c in range(8 * nslot):
                t[off[q] + c * cs[q]: off[q] + c * cs[q] + n] = ((((l * 100 + c) * 1000 + i) * 1000 + j) * 1000 + k).reshape(-1)
        touts.append(torch.from_numpy(t))
    d = os.path.join(tmp, f"r{rank}_{len(H.levels[0].boxes)}_{nslot}")
    bench.dump_outputs(d, torch, "cpu", Hfile, dls, touts, nslot)
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}, sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_sample_reads_the_right_cells_on_any_tiling(tmp_path, monkeypatch):
    from peleanalysis_amd import dist as padist
    from peleanalysis_amd.hierarchy import nested_hierarchy, retile_hierarchy
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)  # a sample smaller than the levels
    Hf = nested_hierarchy(64, 3, 16, is_per=(1, 1, 0))
    H = retile_hierarchy(Hf)
    assert [lv.nboxes for lv in H.levels] != [lv.nboxes for lv in Hf.levels]
    a, na = _encoded_dump(bench, str(tmp_path), Hf, Hf, None, 0, 1)
    b, nb = _encoded_dump(bench, str(tmp_path), Hf, H, None, 0, 1)
    assert sorted(a) == sorted(f"level{l}_{n}.npy" for l in range(3) for n in bench.OUT_FIELDS) == sorted(b)
    assert na <= (1 << 20) + 24 * 128 and nb == na
    for f in a:
        assert a[f].dtype == np.float64 and not np.isnan(a[f]).any() and np.array_equal(a[f], b[f]), f
        l, c = int(f[5]), bench.OUT_FIELDS.index(f[7:-4])
        assert np.all(a[f] // 1e9 == l * 100 + c), f  # level and component of every value
        cells = a[f] % 1e9
        assert len(np.unique(cells)) == len(cells) > 1000  # distinct cells (the sample is deduplicated)
    owners = padist.shard(H, 4)
    parts = [_encoded_dump(bench, str(tmp_path), Hf, H, owners, r, 1)[0] for r in range(4)]
    for f in b:
        assert np.array_equal(np.sort(np.concatenate([p[f] for p in parts])), np.sort(b[f])), f
    # two output slots, every cell of a small level, within the default budget
    monkeypatch.setattr(bench, "DUMP_BYTES", 48 << 20)
    Hf = nested_hierarchy(32, 3, 16, is_per=(1, 1, 0))
    s, ns = _encoded_dump(bench, str(tmp_path), Hf, retile_hierarchy(Hf), None, 0, 2)
    assert len(s) == 48 and len(s["level2_slot1_curv.npy"]) == Hf.levels[2].ncells and ns <= 64 << 20
    assert np.all(s["level2_slot1_curv.npy"] // 1e9 == 215)


def _run(d, *extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "PA_BENCH_REHEARSE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", d] + list(extra), cwd=ROOT,
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0]), {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_the_oracle_computes(tmp_path):
    """a plain run at base 32 writes its dump and nothing of --full into its line; the dump is, bit for bit, the oracle's grad +
    curvature pipelines on bench.py's own inputs (regenerated here with the same seeds on the same internal tiling) put through
    the same sampling"""
    from oracle import oracle as O
    from peleanalysis_amd.hierarchy import MultiFab, mf_layout, nested_hierarchy, retile_hierarchy
    bench = _bench()
    r, got = _run(str(tmp_path / "gpu"), "--steps", "3", "--warmup", "1", "--base", "32", "--box", "16")
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["unit"] == "Mcells/s" and r["dtype"] == "f64"
    assert r["higher_is_better"] is True and r["roofline"]["launches"] >= 3
    for k in ("secondary", "cpu_baseline", "parity_check", "breakdown_ms_per_step"):
        assert k not in r, k  # --full only
    assert len(got) == 24 and all(v.dtype == np.float64 and len(v) > 1000 for v in got.values())
    Hf = nested_hierarchy(32, 3, 16, is_per=(1, 1, 0))
    H = retile_hierarchy(Hf, nranks=1)
    dev = torch.device("cuda", 0)
    states = []
    for li, lv in enumerate(H.levels):  # bench.py main(): the state multifabs of rank 0
        off, cs, tot = mf_layout(lv.boxes, 1, 2)
        t = torch.zeros(tot, dtype=torch.float64, device=dev)
        bench.fill_level_on_device(torch, lv, t, 1, 2, off, cs, dev, 1234 + li)
        states.append(MultiFab(lv, 1, 2, t.cpu().numpy()))
    O.build()
    bc = O.bc_from_flags((1, 1, 0))
    og = [MultiFab(lv, 4, 0) for lv in H.levels]
    oc = [MultiFab(lv, 5, 0) for lv in H.levels]
    O.grad_pipeline(H.levels, [s.copy() for s in states], 0, bc, og, 0)
    O.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oc, 0, MultiFab, prog_min=300.0, prog_max=2000.0)
    touts = []
    for l, lv in enumerate(H.levels):
        m = MultiFab(lv, 8, 0)
        for b in range(lv.nboxes):
            for gc, (ref, rc) in enumerate(((og, 0), (og, 1), (og, 2), (og, 3), (oc, 2), (oc, 3), (oc, 4), (oc, 1))):
                m.valid(b)[gc] = ref[l].valid(b)[rc]
        touts.append(torch.from_numpy(m.data))
    d = str(tmp_path / "oracle")
    bench.dump_outputs(d, torch, "cpu", Hf, [types.SimpleNamespace(level=lv) for lv in H.levels], touts, 1)
    want = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(want) == sorted(got)
    for f in want:
        assert np.array_equal(got[f].view(np.int64), want[f].view(np.int64)), f
