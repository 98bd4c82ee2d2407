"""Streamline tracer (partStream.cpp / StreamPC.cpp): what pins the oracle restatement (AMReX's particle
Redistribute is absent here: parity unpinned) -- a uniform field gives straight lines of arc length dt per
step in both directions; a solid rotation keeps the radius to RK4 accuracy; on an AMR hierarchy the lines
cross coarse-fine interfaces, which triggers the lazy global re-assignment; the field near a wall is cut.
Each answer is written once and asked of all three implementations: the oracle, the numpy restatement
(tests/stream_ref.py) and the kernel (field prepared and lines traced on the device; GPU tier)."""
import numpy as np
import pytest

import stream_cases as SC

from peleanalysis_amd.hierarchy import MultiFab, nested_hierarchy, fill_analytic


def _fields(H, fx, fy, fz):
    out = []
    for lv in H.levels:
        m = MultiFab(lv, 3, 0)
        for c, f in enumerate((fx, fy, fz)):
            fill_analytic(m, c, f)
        out.append(m)
    return out


def _uniform(run):
    H = nested_hierarchy(16, 2, 8, is_per=(0, 0, 0))
    one = lambda x, y, z: 0 * x + 0 * y + 0 * z
    fields = _fields(H, lambda x, y, z: one(x, y, z) + 3.0, lambda x, y, z: one(x, y, z) + 4.0, lambda x, y, z: one(x, y, z) + 12.0)
    seeds = np.array([[0.5, 0.5, 0.5], [0.31, 0.62, 0.44]])
    dt = 0.1 / 32
    pos, nred = run(H, fields, (0, 1, 2), 3, seeds, 20, dt)
    unit = np.array([3.0, 4.0, 12.0]) / 13.0
    for s in range(2):
        for sgn, line in ((+1, pos[2 * s]), (-1, pos[2 * s + 1])):
            want = seeds[s][None, :] + sgn * dt * np.arange(20)[:, None] * unit[None, :]
            assert np.abs(line - want).max() < 1e-14


def _rotation(run):
    H = nested_hierarchy(32, 3, 16, is_per=(0, 0, 0))
    fields = _fields(H, lambda x, y, z: -(y - 0.5) + 0 * x + 0 * z, lambda x, y, z: (x - 0.5) + 0 * y + 0 * z, lambda x, y, z: 0 * x + 0 * y + 0 * z)
    seeds = np.array([[0.5 + 0.2, 0.5, 0.5], [0.5, 0.5 + 0.09, 0.47], [0.5 + 0.33, 0.5, 0.52]])
    dt = 0.4 / 128  # hRK = 0.4 on the finest level
    pos, nred = run(H, fields, (0, 1, 2), 3, seeds, 300, dt)
    r = np.sqrt((pos[..., 0] - 0.5) ** 2 + (pos[..., 1] - 0.5) ** 2)
    # trilinear interpolation of a linear field is exact (away from piecewise-constant coarse-fine ghosts): circles
    assert np.abs(r[0] - 0.2).max() < 2e-4 and np.abs(r[4] - 0.33).max() < 2e-4 and np.abs(pos[:, :, 2] - pos[:, :1, 2]).max() == 0.0
    # forward and backward lines of a seed run in opposite senses by the same arc length
    assert np.abs(np.linalg.norm(np.diff(pos[0], axis=0), axis=1) - dt).max() < 1e-7  # chord of an arc of length dt
    assert nred >= 2  # the r = 0.2 circle crosses the level-1/level-2 interface (0.125) ... at least two re-assignments happen


def _wall(run):
    H = nested_hierarchy(16, 1, 8, is_per=(0, 0, 0))
    one = lambda x, y, z: 0 * x + 0 * y + 0 * z
    fields = _fields(H, lambda x, y, z: one(x, y, z) + 1.0, one, one)
    # interior cells only: the line runs in +x until the ghost layer outside the wall (field 0 there) bends the interpolant
    pos, _ = run(H, fields, (0, 1, 2), 2, np.array([[0.8, 0.5, 0.5]]), 40, 0.02)
    assert np.all(np.diff(pos[0, :, 0]) >= 0) and pos[0, -1, 0] <= 1.0 - 1e-10 and pos[0, -1, 0] > 0.95
    assert np.all(pos[1, :, 0] >= 1e-10)


ANSWERS = {"uniform": _uniform, "rotation": _rotation, "wall": _wall}


@pytest.mark.parametrize("impl", ["oracle", "restatement", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("answer", list(ANSWERS))
def test_known_answer(request, oracle, impl, answer):
    ANSWERS[answer](SC.tracer(impl, oracle, request))


# the three answers under the names they have always had (the oracle's)
def test_uniform_field_straight_lines(oracle):
    _uniform(SC.tracer("oracle", oracle))


def test_rotation_keeps_radius_and_crosses_levels(oracle):
    _rotation(SC.tracer("oracle", oracle))


def test_wall_cut_and_clamp(oracle):
    _wall(SC.tracer("oracle", oracle))
