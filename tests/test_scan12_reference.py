"""CPU: the prefilter's bound with 12-bit row copies against the oracle's fp32 chain, on the adversarial data of
tests/scan12_reference.py.  s is `oracle.pair_distances` (the contract's chain), s~ the model's approximate score, B_ref
the unchanged formula in float64 fed with the 12-bit copies' R, X', X.

Bounds asserted here and where they come from: |s - s~| <= B_ref is the claim itself; rho >= 0.9 of the aligned d = 64
cases is the fp16 suite's figure (the same rows: one fp16 ulp of [2^13, 2^14) is one step of the 12-bit grid; the g terms
take 4 % there); the window table's tolerances are stated at the test."""
import numpy as np
import pytest

import scan12_reference as s12
import scan16_reference as sr
from scan16_reference import IP
from test_plan_cpu import plan_check  # noqa: F401  (the module's fixture: plan_check built for the host)

CASES = s12.all_cases()


def _exact(oracle, c):
    nq, nb = len(c.xq), len(c.xb)
    qi, ri = np.divmod(np.arange(nq * nb, dtype=np.int64), nb)
    return oracle.pair_distances(c.xb, c.xq, qi, ri, IP).reshape(nq, nb)


@pytest.fixture(scope="module")
def exact(oracle):
    memo = {}

    def get(name):
        if name not in memo:
            memo[name] = _exact(oracle, CASES[name])
        return memo[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_bound_is_sound(name, exact):
    c = CASES[name]
    d = c.xb.shape[1]
    B = s12.bound(c.xq, s12.stats(c.xb), sr.pad(d, 32), sr.pad(d, 64))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(exact(name).astype(np.float64) - s12.approx_scores(c.xb, c.xq).astype(np.float64))
    fin = np.isfinite(B)
    worst = (err[fin] / B[fin, None]).max() if fin.any() else 0.0
    print(f"{name}: max |s - s~| / B_ref = {worst:.4f}" + ("" if fin.all() else "  (B not finite for some queries)"))
    assert np.isfinite(err[fin]).all() and worst <= 1.0


def test_copy_format():
    """the copy itself: integers of 12 bits, ties to even, the clamp at 2047, the exponent clamp, entries that round to 0"""
    x = np.array([[1024.5, 1025.5, -2047.5, 0.49, -0.5, 0.5000001, 2046.5, 3.0]], np.float32) * np.float32(2.0 ** -3)
    n, e = s12.copies(x)
    assert e[0] == -3 and n[0].tolist() == [1024.0, 1026.0, -2047.0, 0.0, -0.0, 1.0, 2046.0, 3.0]
    n, e = s12.copies(np.array([[2047.75, 1.0]], np.float32))  # rounds to 2048: clamped
    assert e[0] == 0 and n[0].tolist() == [2047.0, 1.0]
    n, e = s12.copies(np.array([[2.0 ** -120, 2.0 ** -129]], np.float32))  # below the exponent clamp: 2^-120 = 2^8 2^-128
    assert e[0] == -128 and n[0].tolist() == [256.0, 0.0]
    c = CASES["clamped_max_d64"]
    n, e = s12.copies(c.xb[c.expect["clamped"]])
    assert (n[:, 0] == 2047).all()
    x = c.xb[c.expect["clamped"]].astype(np.float64)
    assert (np.abs(x - s12.restored(n, e))[:, 0] * 2.0 ** -e.astype(np.float64) >= 0.5).all()  # more than rounding alone leaves
    c = CASES["rounds_to_zero_fits"]
    n, _ = s12.copies(c.xb[c.expect["flushed"]])
    assert (n[:, 1:] == 0).all() and (n[:, 0] >= 1024).all()
    assert (s12.approx_scores(c.xb, c.xq)[:, c.expect["flushed"]] == 0).all()
    n, e = s12.copies(CASES["tiny_d64"].xb)
    assert (e == -128).sum() > 100 and ((np.abs(n).max(1) < 1024) & (np.abs(n).max(1) > 0)).any()  # clamped rows lose bits


@pytest.mark.parametrize("name", ["aligned_rows_d64", "aligned_query_d64"])
def test_aligned_cases_reach_the_edge(name, exact):
    """the victim belongs to the exact top-k, the decoys do not, the approximate order says the opposite, the victim sits at
    rho >= 0.9 of the window -- and a bound 10 % short leaves it outside"""
    c = CASES[name]
    q, v = c.expect["query"], c.expect["victim"]
    s = exact(name)[q].astype(np.float64)
    top = set(np.argsort(-s, kind="stable")[:c.k].tolist())
    assert v in top and not (set(c.expect["decoys"]) & top)
    p = s12.predict(c.xb, c.xq, c.k)
    o = p["queries"][q]
    atop = set(np.argsort(-p["approx"][q].astype(np.float64), kind="stable")[:c.k].tolist())
    assert v not in atop and c.expect["decoys"][0] in atop
    rho = (-float(p["approx"][q, v]) - o["t"]) / (2.0 * o["B"])
    print(f"{name}: rho = {rho:.4f}, candidates_max {p['candidates_max']}")
    assert 0.9 <= rho <= 1.0
    assert not p["fallback"] and v in o["inside"] and p["candidates_max"] == c.expect["candidates_max"]
    s12.assert_robust(p, name)
    short = s12.predict(c.xb, c.xq, c.k, bscale=0.9)
    assert v not in short["queries"][q]["inside"]


@pytest.mark.parametrize("name", list(CASES))
def test_predictions(name):
    """what each case's searches must do with 12-bit copies, and that the library's round-up margins cannot change it"""
    c = CASES[name]
    p = s12.predict(c.xb, c.xq, c.k)
    print(f"{name}: fallback {p['fallback']}, candidates_max {p['candidates_max']}")
    # (gate_pass: rows of one magnitude carry an exponent 3 above the fp16 copies', so its e_q + EMAX = 83 passes the unchanged
    # gate of 80 no longer: it falls back, like gate_over)
    if c.expect.get("fallback") is not None and name != "gate_pass":
        assert p["fallback"] == c.expect["fallback"]
    if name == "rounds_to_zero_fits":
        assert p["candidates_max"] == c.expect["candidates_max"]
    if name in s12.ROBUST:
        s12.assert_robust(p, name)


def test_kprime():
    assert [s12.kprime(k) for k in (1, 64, 100, 682, 683, 1920, 1921, 2047, 2048)] == [129, 192, 300, 2046, 2048, 2048, 2048, 2048, 2048]


def test_planner_agrees(plan_check):  # noqa: F811
    """`plan_check s16`: the planner's k' of both formats is the models', and k' = k is not eligible"""
    import subprocess
    ks = (1, 64, 100, 682, 683, 1920, 2047, 2048)
    r = subprocess.run([str(plan_check), "s16"], input="".join(f"300000 32 {k} 0\n" for k in ks), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(ks)
    for k, line in zip(ks, lines):
        assert line == (f"300000 32 {k} 0: fp16 kprime {sr.kprime(k)} eligible {int(sr.kprime(k) > k)}, "
                        f"12-bit kprime {s12.kprime(k)} eligible {int(s12.kprime(k) > k)}"), line


def test_window_estimate():
    """DESIGN 4.9's table: 20 000 normalised gaussian rows at d = 1024, extrapolated to 10 M rows, k = 100.  R is a maximum
    over the sample and the figures move a few percent with it: 15 % around the table's entries, which are rounded.  The
    12-bit window must leave k' - k = 200 half empty even at 1.5 times its expectation (what the fp16 path's measured
    maximum was of its own)."""
    rng = np.random.default_rng(0)
    xb = rng.standard_normal((20000, 1024)).astype(np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    xq = rng.standard_normal((32, 1024)).astype(np.float32)
    xq /= np.linalg.norm(xq, axis=1, keepdims=True)
    h, e = sr.copies(xb, -128)
    n, e12 = s12.copies(xb)
    rows = {"fp16": (sr.restored(h, e), 2.3e-4, 7.6e-4, 24), "12-bit": (s12.restored(n, e12), 1.18e-3, 1.7e-3, 62),
            "fp16 cut to 7 bits": (s12.quantize_fp16_bits(xb, 7), 3.8e-3, 4.3e-3, 231), "10-bit": (s12.fixed_point(xb, 10), 4.7e-3, 5.3e-3, 327),
            "8-bit": (s12.fixed_point(xb, 8), 1.9e-2, 2.0e-2, 12800)}
    got = {}
    for name, (xp, R0, B0, W0) in rows.items():
        R, B, W = s12.window_estimate(xp, xb, xq)
        got[name] = W
        print(f"{name}: R = {R:.3g} (table {R0:.3g}), B_q = {B:.3g} ({B0:.3g}), rows beyond the k-th = {W:.0f} ({W0})")
        assert abs(R / R0 - 1) < 0.15 and abs(B / B0 - 1) < 0.15 and abs(W / W0 - 1) < 0.15
    assert np.allclose(s12.fixed_point(xb, 12), s12.restored(n, e12))
    assert 1.5 * got["12-bit"] < (s12.kprime(100) - 100) / 2
    assert got["8-bit"] > 2048  # more than a selection carries
