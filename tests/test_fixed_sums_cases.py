"""CPU tier: the inputs of tests/test_gpu_fixed_sums.py can SEE the low limbs of the fixed-point sums.  The visibility condition of
DESIGN.md 3.7 is a condition on the inputs: it is asserted here on the restatements' terms and the big-integer model alone, so a set
of cases that could not notice a lost carry fails before any kernel runs."""
import math

import numpy as np
import pytest

import fixed192_ref as F
import fixed_sums_cases as C


@pytest.mark.parametrize("kernel", ["jpdf", "condmean", "integral"])
def test_visibility_condition(kernel):
    """over the cancel, cancel_tail, ties and chains cases of the kernel, every accumulator of every non-empty bin counted on its own: at least a quarter hold a sum below
    2^(k-100) (wholly inside limb 0), at least a quarter one in 2^(k-93) .. 2^(k-40) (its mantissa straddles limbs 0 / 1), and every
    case has a bin whose exact sum is negative"""
    (n, tiny, mid), no_negative = C.pooled_visibility(kernel)
    print(f"{kernel}: {n} sums in non-empty bins, {tiny} inside limb 0, {mid} across limbs 0 / 1")
    assert n > 0 and 4 * tiny >= n and 4 * mid >= n, (n, tiny, mid)
    assert not no_negative, f"cases without a negative sum: {no_negative}"


@pytest.mark.parametrize("family", C.VISIBLE)
def test_families_realise_their_classes(family):
    """one variable, groups of 9 cells with weights 1 and 1/8: the terms w * v are exact and the group sums land where their class says"""
    ngroups, k = 60, 5
    gid = np.repeat(np.arange(ngroups), 9)
    w = np.tile([1.0, 1.0, 1.0, 1.0, 1.0, 0.125, 0.125, 0.125, 0.125], ngroups)
    cls = gid % 3
    v = C.family_values(family, gid, w, cls, k, seed=3, sign=1 - 2 * (gid % 2))
    sums = F.sum_by_bin(gid, w * v, 157 - k, ngroups)
    assert F.converts_exactly(w * v, 157 - k)
    for g, s in enumerate(sums):
        assert F.read(s, 157 - k) == math.fsum((w * v)[gid == g].tolist())
        if g % 3 == 0:
            assert abs(s) < 1 << 57, (g, s)
        elif g % 3 == 1:
            assert 1 << 64 <= abs(s) < 1 << 117 and (family == "chains" or (s < 0) == (g % 2 == 1)), (g, s)
    assert np.abs(v).max() < 2.0 * C.A


def test_every_launcher_path_is_among_the_cases():
    """the tables and wavefront sums the launchers choose for the cases, restated from their conditions"""
    modes = {C.condmean_mode(nb, na, mm, unc) for _, na, nb, mm, _ in C.CONDMEAN_CASES for unc in (False, True)}
    assert modes == {0, 1, 2}
    for _, na, nb, mm, want in C.CONDMEAN_CASES:
        assert C.condmean_mode(nb, na, mm, False) == want
    H = C.hierarchies()
    paths = set()
    for h, kind, dir_, nv, fam, sq, cond in C.integral_cases():
        nrows = 1 + (nv + (1 if cond else 0)) * (2 if sq else 1)
        paths |= C.integral_paths(H[h], kind, dir_, nrows, False) | C.integral_paths(H[h], kind, dir_, nrows, True)
    assert paths == {("end", 2), ("tile", 2), ("none", 2), ("step", 1), ("none", 1), ("none", 0)}
    assert C.integral_paths(H["wide"], 2, 1, 4, False) == {("tile", 1)}                     # rows of whole wavefronts: straight to the global table
    assert ("none", 1) in C.integral_paths(H["tall"], 2, 0, 17, False)                       # a table beyond PA_INT_LDS_MAX
    assert ("tile", 1) in C.integral_paths(H["tall"], 2, 1, 17, False)
