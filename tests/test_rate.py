"""The target-bitrate rules on the host (rate.h through cairo_rate_estimate,
cairo_rate_init and cairo_rate_step): the integer estimate
against a big-integer model and against real payloads, the control law against
a model of its definition (include/cairo_amd.h), its behaviour on CIF band4
through tools/rate_sim.py, and the ABI.  No GPU."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from tools import rate_sim

EVX_ERROR_INVALID_ARGS = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- models: Python integers, written from the definition -------------------
def log2_q16(x: int) -> int:
    assert 1 <= x < 1 << 32
    e = x.bit_length() - 1
    y = x << (31 - e)
    bits = 0
    for _ in range(16):
        y = (y * y) >> 31
        b = 1 if y >= 1 << 32 else 0
        bits = (bits << 1) | b
        if b:
            y >>= 1
    return (e << 16) | bits


def estimate(n: int, z: int) -> int:
    term = lambda v: v * log2_q16(v) if v else 0  # noqa: E731
    return (term(n) - term(z) - term(n - z)) >> 16  # an arithmetic shift, as int64's


def div0(a: int, b: int) -> int:
    """Division toward zero."""
    return abs(a) // b if a >= 0 else -(abs(a) // b)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class Law:
    """The control law of include/cairo_amd.h on a dict state."""

    def __init__(self, T, q0=8, qmin=1, qmax=31, W=32):
        self.T, self.q0, self.qmin, self.qmax, self.W = T, q0, qmin, qmax, W
        self.debt, self.P, self.O, self.launches = 0, None, None, 0
        self.aim = 0

    def step(self, n_new, obs_sum):
        T = self.T
        q, aim = self.q0, T
        if self.launches >= 2:
            P, O = self.P, self.O
            self.debt = clamp(self.debt + obs_sum - O["n"] * T, -(1 << 60), 1 << 60)
            dp = self.debt + P["n"] * (P["aim"] - T)
            aim = clamp(T - div0(dp, self.W), max(T // 4, 1), 4 * T)
            M = obs_sum // O["n"]
            s = max(0, max(M, aim).bit_length() - 24)
            m, t = M >> s, max(aim >> s, 1)
            qm = (O["q"] * m * m + t * t // 2) // (t * t)
            st = 1 + P["q"] // 4
            q = clamp(qm, P["q"] - st, P["q"] + st)
        q = clamp(q, self.qmin, self.qmax)
        self.O, self.P = self.P, dict(n=n_new, q=q, aim=aim)
        self.launches += 1
        self.aim = aim
        return q


# ---- the estimate -----------------------------------------------------------
def test_estimate_equals_model(cairo):
    rng = random.Random(20)
    pairs = []
    for n in (0, 1, 2, 31, 32, 33, 1 << 29):
        pairs += [(n, 0), (n, n), (n, n // 2)]
    pairs += [((1 << 32) - 1, 0), ((1 << 32) - 1, 1), ((1 << 32) - 1, (1 << 31))]
    for _ in range(400):
        n = rng.randrange(1, 1 << rng.randrange(1, 33))
        pairs.append((n, rng.randrange(0, n + 1)))
    for n, z in pairs:
        assert cairo.rate_estimate(n, z) == estimate(n, z), (n, z)
    # the logarithm itself, where its sixteen bits are known: exact powers, and 3 = 2^1.58496...
    assert log2_q16(1) == 0 and log2_q16(1 << 31) == 31 << 16
    assert log2_q16(3) == int(np.floor(np.log2(3.0) * 65536))
    L = cairo.lib()
    assert L.cairo_rate_estimate(1 << 32, 0) == -1 and L.cairo_rate_estimate(5, 6) == -1


CASES = [("band4", 16, 16), ("band4", 64, 48), ("band4", 352, 288), ("noise", 352, 288), ("static", 352, 288),
         ("black", 352, 288)]


@pytest.fixture(scope="module")
def payload_runs(orc, cairo):
    """(kind, w, h, q) -> the simulation's records of four frames at a fixed q (computed once)."""
    out = {}
    for kind, w, h in CASES:
        frames = rate_sim.make_frames(kind, w, h, 4)
        for q in (1, 16, 31):
            out[kind, w, h, q] = rate_sim.simulate(frames, [4], 4, fixed_q=q)
    return out


def test_estimate_against_real_payloads(payload_runs):
    """Oracle encode -> host precode -> popcount -> E, against the oracle's
    payload bits: |payload - E| <= 64 + (N >> 15).  Measured (all 72 frames,
    N from 147 to 691 411 bits): payload - E from 0 to +17; DESIGN.md §4.20
    has a wider sweep at 1280x720 (-21 .. +43, N up to 6.3 M)."""
    lo, hi = 0, 0
    for key, recs in payload_runs.items():
        for t, r in enumerate(recs):
            e = r["est_bits"] - rate_sim.FRAME_RECORD_BITS
            d = r["payload_bits"] - e
            lo, hi = min(lo, d), max(hi, d)
            assert abs(d) <= 64 + (r["feed_bits"] >> 15), f"{key} frame {t}: payload {r['payload_bits']} vs E {e} (N {r['feed_bits']})"
    ns = [r["feed_bits"] for v in payload_runs.values() for r in v]
    print(f"payload - E over {len(ns)} frames (N {min(ns)} .. {max(ns)}): {lo} .. {hi}")


# ---- the law ----------------------------------------------------------------
def _run_both(cairo, cfg, seq):
    """seq: (n_new, obs_sum) per launch -> [(q, aim, debt)] of model and library, compared."""
    law = Law(cfg["target_bits"], cfg["q0"], cfg["qmin"], cfg["qmax"], cfg["window"])
    lib = cairo.RateModel(**cfg)
    out = []
    for k, (n, obs) in enumerate(seq):
        want = (law.step(n, obs), law.aim, law.debt)
        got = (lib.step(n, obs), lib.aim, lib.debt)
        assert got == want, f"{cfg} launch {k} ({n}, {obs}): library {got}, model {want}"
        out.append(got)
    return out


def test_law_equals_model_random(cairo):
    rng = random.Random(7)
    for trial in range(300):
        T = rng.choice([1, 2, 1000, 55000, 400000, 1 << 20, (1 << 28) - 1, 1 << 28])
        qmin = rng.randrange(1, 32)
        qmax = rng.randrange(qmin, 32)
        cfg = dict(target_bits=T, q0=rng.randrange(1, 32), qmin=qmin, qmax=qmax, window=rng.choice([1, 2, 16, 32, 1000]))
        scale = rng.choice([0.01, 0.3, 1.0, 3.0, 100.0])
        seq = []
        for _ in range(rng.randrange(1, 40)):
            n = rng.randrange(1, 49)
            obs = rng.choice([0, int(n * T * scale * rng.random() * 2), rng.randrange(0, 1 << 41)])
            seq.append((n, min(obs, 1 << 48)))
        _run_both(cairo, cfg, seq)


def test_law_named_cases(cairo):
    base = dict(target_bits=50000, q0=8, qmin=1, qmax=31, window=32)
    # the first two launches: q0 and aim T whatever is passed as observation
    r = _run_both(cairo, base, [(4, 123456789), (3, 0)])
    assert [x[0] for x in r] == [8, 8] and [x[1] for x in r] == [50000, 50000] and r[1][2] == 0
    # debt of both signs
    r = _run_both(cairo, base, [(4, 0), (4, 0), (4, 4 * 80000), (4, 4 * 80000)])
    assert r[2][2] == 4 * 30000 and r[2][1] < 50000 and r[2][0] > 8
    r = _run_both(cairo, base, [(4, 0), (4, 0), (4, 4 * 20000), (4, 4 * 20000)])
    assert r[2][2] == -4 * 30000 and r[2][1] > 50000 and r[2][0] < 8
    # aim at both clamps (a short window), q at qmin and qmax
    tight = dict(base, window=1, qmin=6, qmax=10)
    r = _run_both(cairo, tight, [(4, 0), (4, 0)] + [(4, 4 * 10 ** 6)] * 6)
    assert r[-1][1] == 50000 // 4 and r[-1][0] == 10
    r = _run_both(cairo, tight, [(4, 0), (4, 0)] + [(4, 400)] * 6)
    assert r[-1][1] == 4 * 50000 and r[-1][0] == 6
    # the step limit binds in both directions: from 8 by at most 1 + 8 / 4 = 3 per launch
    r = _run_both(cairo, base, [(4, 0), (4, 0), (4, 4 * 10 ** 7), (4, 4 * 10 ** 7)])
    assert [x[0] for x in r] == [8, 8, 11, 14]
    r = _run_both(cairo, base, [(4, 0), (4, 0), (4, 400), (4, 400)])
    assert [x[0] for x in r] == [8, 8, 5, 3]
    # T = 1 and T = 2^28; an observation near 2^40
    _run_both(cairo, dict(base, target_bits=1), [(1, 0), (1, 0), (1, 80), (1, 80), (48, 1 << 40), (2, 0), (2, 3)])
    _run_both(cairo, dict(base, target_bits=1 << 28),
              [(48, 0), (48, 0), (48, 48 << 28), (48, (1 << 40) - 1), (48, 1 << 40), (1, 0), (1, 1 << 30)])


def test_law_behaviour_cif_band4(cairo):
    """CIF band4, 64 frames in launches of 4, T = the measured mean of the
    fixed q = 12 encode: the controlled mean lies between the fixed-quality
    means at the smallest and the largest quality the run used after its first
    four launches (a bracket from the oracle, not from the controller)."""
    frames = rate_sim.make_frames("band4", 352, 288, 64)
    launches = rate_sim.launches_of(64, 4)
    mean = lambda recs: float(np.mean([r["payload_bits"] + rate_sim.FRAME_RECORD_BITS for r in recs]))  # noqa: E731
    T = int(round(mean(rate_sim.simulate(frames, launches, 4, fixed_q=12))))
    recs = rate_sim.simulate(frames, launches, 4, rate=dict(target_bits=T, q0=8, qmin=1, qmax=31, window=32))
    qs = rate_sim.summary(recs)[0]
    lo_q, hi_q = min(qs[4:]), max(qs[4:])
    most = mean(rate_sim.simulate(frames, launches, 4, fixed_q=lo_q))
    least = most if hi_q == lo_q else mean(rate_sim.simulate(frames, launches, 4, fixed_q=hi_q))
    got = mean(recs)
    print(f"T {T}: controlled mean {got:.0f}, q per launch {qs}; fixed q={lo_q}: {most:.0f}, q={hi_q}: {least:.0f}")
    assert least <= got <= most, f"mean {got:.0f} outside [{least:.0f}, {most:.0f}] (q {hi_q} .. {lo_q})"


# The runtimes are linked into the program, so nothing is preloaded.
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def test_rules_sanitized(tmp_path):
    """rate.h with a plain host compiler, under the address and undefined-behaviour
    sanitizers, at the ends of every range the entry points accept."""
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build rate_host_main")
    exe = str(tmp_path / "rate_host_main")
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", exe, os.path.join(ROOT, "tests/sanitize/rate_host_main.cpp")],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr[-4000:]
    assert run.stdout.split()[0] == "steps"


# ---- ABI ----------------------------------------------------------------------
def test_abi_sizes_and_refusals(cairo):
    import cairo_amd as ca

    L = cairo.lib()
    assert L.cairo_rate_size() == ctypes.sizeof(ca._Rate) == 32
    assert L.cairo_rate_state_size() == ctypes.sizeof(ca._RateState) == 48
    assert L.cairo_rate_info_size() == ctypes.sizeof(ca._RateInfo) == 48
    good = dict(target_bits=1000, q0=8, qmin=1, qmax=31, window=32)
    ca.RateModel(**good)
    for bad in (dict(target_bits=0), dict(target_bits=(1 << 28) + 1), dict(q0=0), dict(q0=32), dict(qmin=0),
                dict(qmax=32), dict(qmin=9, qmax=8), dict(window=0)):
        with pytest.raises(cairo.CairoError) as e:
            ca.RateModel(**dict(good, **bad))
        assert e.value.status == EVX_ERROR_INVALID_ARGS, bad
    cfg, st = ca._Rate(1000, 8, 1, 31, 32), ca._RateState()
    cfg.reserved[1] = 1
    assert L.cairo_rate_init(ctypes.byref(st), ctypes.byref(cfg)) == EVX_ERROR_INVALID_ARGS
    # a refused step leaves the state as it was
    m = ca.RateModel(**good)
    m.step(4), m.step(4), m.step(4, 9000)
    before = bytes(m.state)
    for n, obs in ((0, 0), (65536, 0), (4, -1), (4, (1 << 48) + 1)):
        with pytest.raises(cairo.CairoError):
            m.step(n, obs)
    q = ctypes.c_uint32()
    assert L.cairo_rate_step(ctypes.byref(m.state), ctypes.byref(cfg), 4, 0, ctypes.byref(q)) == EVX_ERROR_INVALID_ARGS
    assert bytes(m.state) == before
