"""CPU tier: the host half of peleanalysis_amd/csrc/pa_fixed192.h (to_fixed, u192_add, u192_mul, from_fixed, scale_of) against the
big-integer model of tests/fixed192_ref.py.  tests/fixed192_host.hip is a stand-alone program around the header; it is built twice --
plain, and with the address and undefined-behaviour sanitizers on the host code -- and both must reproduce the model on every list:
the three limbs with ==, the bits of the rounded result with ==, and == math.fsum where every term converts exactly."""
import math
import os
import random
import shutil
import subprocess
from fractions import Fraction

import pytest

import fixed192_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "peleanalysis_amd", "csrc")
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def _hipcc():
    cc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return cc if os.path.exists(cc) else shutil.which("hipcc")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def program(request, tmp_path_factory):
    cc = _hipcc()
    if cc is None:
        pytest.skip("hipcc is not installed")
    exe = str(tmp_path_factory.mktemp("fx192") / ("fixed192_host_" + request.param))
    cmd = [cc, "--offload-arch=gfx950", "-O1", "-g", "-I", CSRC, os.path.join(HERE, "fixed192_host.hip"), "-o", exe] + (SAN if request.param == "sanitized" else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


def _run(exe, records):
    r = subprocess.run([exe], input="\n".join(records) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stderr[-4000:]}"
    lines = r.stdout.splitlines()
    assert len(lines) == len(records), (len(lines), len(records), r.stderr[-2000:])
    return lines


# ----------------------------------------------------------------------------- the lists
def Q(i, s):
    """i quanta (units of 2^-s) as a double; i must be representable"""
    v = math.ldexp(float(i), -s)
    assert Fraction(v) * Fraction(2) ** s == i
    return v


def mant(rng):
    return rng.getrandbits(52) | (1 << 52)


CHAIN_A, CHAIN_B = F.CHAIN_A, F.CHAIN_B


def chain_terms(a, b, sign, s):
    """sign * (2^a - 2^b) quanta: one double where it is one, else the two terms whose sum it is"""
    if a - b <= 53:
        return [Q(sign * ((1 << a) - (1 << b)), s)]
    return [Q(sign * (1 << a), s), Q(-sign * (1 << b), s)]


def make_lists():
    """-> list of (family, s, terms)"""
    rng = random.Random(192)
    out = []

    def scales(n):
        for _ in range(n):
            k = rng.randint(-300, 200)
            M = math.ldexp(rng.uniform(0.5, 1.0), k)
            assert F.scale_of(M) == 157 - k
            yield k, M, 157 - k

    for k, M, s in scales(400):
        out.append(("uniform", s, [rng.uniform(-M, M) for _ in range(rng.randint(1, 120))]))
    for k, M, s in scales(500):  # 160 binades below M: the low bits of the small terms fall under the quantum, negative ones too
        out.append(("spread", s, [rng.choice((-1, 1)) * math.ldexp(float(mant(rng)), k - 53 - rng.randint(0, 160)) for _ in range(rng.randint(1, 80))]))
    for k, M, s in scales(500):
        t = []
        for _ in range(rng.randint(1, 40)):
            x = rng.uniform(0.25, 1.0) * M * rng.choice((-1, 1))
            res = rng.randrange(3)
            y = x if res == 0 else (math.nextafter(x, 0.0) if res == 1 else x * (1.0 - 2.0 ** -30))
            t += [x, -y]
        rng.shuffle(t)
        out.append(("cancel", s, t))
    for k, M, s in scales(600):  # ties: B + odd half-ulps of B, alone (to even) or with a tail that decides, in both signs
        B = math.ldexp(1.0, k - 1 - rng.randint(0, 60))
        odd = rng.choice((1, 3, 5, 7, (1 << 20) + 1, (1 << 52) - 1))
        sg = rng.choice((-1.0, 1.0))
        t = [sg * B, sg * odd * 2.0 ** -53 * B]
        if rng.random() < 0.67:
            t.append(rng.choice((-1.0, 1.0)) * 2.0 ** -rng.randint(60, 110) * B)
        if rng.random() < 0.3:  # a large pair that cancels around it
            x = rng.uniform(0.5, 1.0) * M
            t += [x, -x]
        rng.shuffle(t)
        out.append(("ties", s, t))
    for k, M, s in scales(8):  # carry and borrow chains across both limb boundaries
        for a in CHAIN_A:
            for b in CHAIN_B:
                if b >= a:
                    continue
                for sg in (1, -1):
                    base = chain_terms(a, b, sg, s)
                    out.append(("chains", s, base))
                    out.append(("chains", s, base + [Q(sg, s)]))          # ... + 1 quantum: the chain of ones carries out
                    out.append(("chains", s, base + [Q(-sg, s)]))
                    a2, b2 = rng.choice(CHAIN_A), rng.choice(CHAIN_B[:4])
                    out.append(("chains", s, base + chain_terms(a2, b2, -sg, s)))
                    out.append(("chains", s, base + chain_terms(a, rng.choice([x for x in CHAIN_B if x < a]), -sg, s)))
    for k, M, s in scales(4):  # a 53-bit mantissa at every shift: q == 0, limb == 1 and the hi word of to_fixed
        for sh in range(0, 106):
            m = mant(rng)
            for sg in (1, -1):
                out.append(("shifts", s, [math.ldexp(float(sg * m), sh - s)]))
            out.append(("shifts", s, [math.ldexp(float(m), sh - s), math.ldexp(float(-mant(rng)), sh - s)]))
    for k, M, s in scales(40):
        out.append(("zeros", s, [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072009e-308, rng.uniform(-M, M)]))
        top = math.ldexp(1.0, k + 1)
        out.append(("edge_accept", s, [math.nextafter(top, 0.0)]))
        out.append(("edge_accept", s, [-math.nextafter(top, 0.0), rng.uniform(-M, M)]))
        out.append(("edge_overflow", s, [top, rng.uniform(-M, M)]))
        out.append(("edge_overflow", s, [-top]))
        out.append(("edge_overflow", s, [top * 4.0, M]))
        out.append(("nonfinite", s, [rng.choice((math.inf, -math.inf, math.nan)), rng.uniform(-M, M)]))
    return out


LISTS = make_lists()


def test_the_model_is_the_design():
    """to_fixed is int(Fraction(t) * 2^s); read rounds once; the families are all there and number a few thousand"""
    rng = random.Random(7)
    for fam, s, terms in rng.sample(LISTS, 300):
        for t in terms:
            v, f = F.to_fixed(t, s)
            if f == 0:
                assert v == int(Fraction(t) * Fraction(2) ** s)
    assert F.read(3, 1) == 1.5 and F.read(-(1 << 60) - 1, 0) == -float(1 << 60) and F.read((1 << 53) + 1, 0) == float(1 << 53)  # tie -> even
    assert F.read((1 << 54) + 6, 0) == float((1 << 54) + 8) and F.read(5, -2) == 20.0
    assert F.scale_of(0.0) == F.scale_of(-1.0) == F.scale_of(math.inf) == F.scale_of(math.nan) == 157 and F.scale_of(1.0) == 156 and F.scale_of(0.75) == 157
    assert F.limbs(-1) == [2 ** 64 - 1] * 3 and F.from_limbs(F.limbs(-12345 << 70)) == -12345 << 70
    assert F.converts_exactly([0.5, -0.25], 2) and not F.converts_exactly([0.125], 2)
    for fam, s, terms in rng.sample(LISTS, 600):
        if all(math.isfinite(t) for t in terms):
            assert F.all_convert_exactly(terms, s) == F.converts_exactly(terms, s), (fam, s)
    fams = {f for f, _, _ in LISTS}
    assert fams == {"uniform", "spread", "cancel", "ties", "chains", "shifts", "zeros", "edge_accept", "edge_overflow", "nonfinite"}
    assert 3000 <= len(LISTS) <= 8000


def test_header_sums_match_the_model(program):
    recs = ["S %d %x " % (s, len(t)) + " ".join("%x" % F.bits(x) for x in t) for _, s, t in LISTS]
    lines = _run(program, recs)
    exact = 0
    for (fam, s, terms), line in zip(LISTS, lines):
        flag, w0, w1, w2, rb = (int(x, 16) for x in line.split())
        tot, mflag = F.sum_terms(terms, s)
        what = f"{fam} s={s} terms={[x.hex() for x in terms]}"
        assert flag == mflag, f"{what}: flags {flag}, model {mflag}"
        assert [w0, w1, w2] == F.limbs(tot), f"{what}: limbs {[hex(w0), hex(w1), hex(w2)]}, model {[hex(x) for x in F.limbs(tot)]}"
        want = F.read(tot, s)
        assert rb == F.bits(want), f"{what}: from_fixed gives bits {rb:#x}, the model {want!r} ({F.bits(want):#x})"
        if fam == "edge_accept":
            assert flag == 0 and F.converts_exactly(terms, s)
        if fam == "edge_overflow":
            assert flag == F.OVERFLOW
        if fam == "nonfinite":
            assert flag == F.NONFINITE
        if flag == 0 and F.converts_exactly(terms, s):
            assert rb == F.bits(math.fsum(terms)), f"{what}: every term converts exactly, but the result is not fsum"
            exact += 1
    assert exact > len(LISTS) // 3


def test_u192_mul_and_scale_of_match_the_model(program):
    rng = random.Random(33)
    cases = []
    for _ in range(600):
        k = rng.randint(-300, 200)
        s = 157 - k
        pick = rng.randrange(4)
        if pick == 0:  # a maximal term: twice the declared bound, less one ulp
            a = F.to_fixed(rng.choice((-1, 1)) * math.nextafter(math.ldexp(1.0, k + 1), 0.0), s)[0]
        elif pick == 1:
            a = rng.choice((-1, 1)) * rng.getrandbits(rng.randint(1, 158))
        elif pick == 2:  # all-ones limbs
            a = rng.choice((-1, 1)) * ((1 << rng.choice((64, 128, 158))) - 1)
        else:
            a = F.to_fixed(rng.uniform(-1, 1) * math.ldexp(1.0, k), s)[0]
        n = rng.choice((0, 1, 2, (1 << 33) - 1, (1 << 32), rng.getrandbits(33), rng.getrandbits(20)))
        cases.append((a, n))
    recs = ["M %x %x %x %x" % (*F.limbs(a), n) for a, n in cases]
    mags = [1.0, 0.75, 0.5, 3.0, 2.0 ** -300, 2.0 ** 200, 5e-324, 0.0, -0.0, -2.0, math.inf, -math.inf, math.nan, 1.7976931348623157e308] + \
           [math.ldexp(rng.uniform(0.5, 1.0), rng.randint(-300, 200)) for _ in range(100)]
    recs += ["K %x" % F.bits(M) for M in mags]
    lines = _run(program, recs)
    for (a, n), line in zip(cases, lines):
        got = [int(x, 16) for x in line.split()]
        assert got == F.limbs(a * n), f"u192_mul({a:#x}, {n:#x}): {[hex(x) for x in got]}, model {[hex(x) for x in F.limbs(a * n)]}"
        if abs(a) < 1 << 158 and n < 1 << 33:  # the stated headroom: 2^33 maximal terms stay clear of the sign bit
            assert F.from_limbs(got) == a * n
    for M, line in zip(mags, lines[len(cases):]):
        assert int(line) == F.scale_of(M), f"scale_of({M!r}): {line}, model {F.scale_of(M)}"
