"""CPU: the 16-bit prefilter's error bound against the oracle's fp32 chain, on the adversarial cases of
tests/scan16_reference.py -- the bound is sound, the cases reach its edge, and the windows they predict are robust.

s is `oracle.pair_distances` (the contract's chain), s~ the model's approximate score, B_ref the formula in float64.

What this suite found.  The bound's last term was a flat 2^-140 ("an ldexp below the normal range").  The fp32 chain rounds
every subnormal partial sum to a multiple of 2^-149, up to 2^-150 per step: `subnormal_scores_d1280` (row 0, query 0: all
1280 products are +2^-150, every step ties to even, s = 0, s~ = 640 * 2^-149) exceeds the parent's bound of
512.54 * 2^-149 by 127.46 * 2^-149.  At d = 1024 the same layout reaches 512 * 2^-149 = 2^-140 exactly and the g terms
(0.35 * 2^-149) keep it inside -- no chain can do more there: 1024 half-steps and the ldexp's half make 512.5, and s - s~ is
a whole multiple of 2^-149.  d = 64 is far inside.  The term is now (dp + 1) 2^-149 (`test_parent_tail_is_violated_at_1280`
keeps the old formula's failure on record).

Reached rho = (v~ - t~) / (2 B_ref) of the victim, derived from the formula and the oracle (printed by the tests):
aligned_rows_d64 0.943, aligned_query_d64 0.946, aligned_rows_d1024 0.567 (the g terms are d (2^-22 + 2^-24) X' / R of
the first term: 4 % at d = 64 with X' / R = 8200 / 3.75, 67 % at d = 1024).  Predicted windows (candidates_max):
aligned rows and query 12 = k - 1 solid rows + the victim + 2 decoys; flushed_fits 54 = all the flushed rows; tiny_d64 11,
subnormal_query_d64 11, subnormal_scores_d64_p125 14, the gate cases 5.

The flushed cases cannot be made tight in B: an entry is flushed only below 2^-27 of the row's largest, and the g terms
weigh the largest with d 2^-22, so they exceed the flushed entries' |q| R by 2^5 / sqrt(d) and more.  What these cases pin
is the copy (approximate scores exactly 0, one tie over all flushed rows) and the window's count."""
import numpy as np
import pytest

import scan16_reference as sr
from scan16_reference import IP

CASES = sr.all_cases()
ULP = 2.0 ** -149


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


@pytest.fixture(scope="module")
def pred():
    memo = {}

    def get(name):
        if name not in memo:
            c = CASES[name]
            memo[name] = sr.predict(c.xb, c.xq, c.k)
        return memo[name]
    return get


def _errors(c, s, tail=None):
    d = c.xb.shape[1]
    B = sr.bound(c.xq, sr.stats(c.xb), sr.pad(d, 32), sr.pad(d, 64), tail)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(s.astype(np.float64) - sr.approx_scores(c.xb, c.xq).astype(np.float64))
    return err, B


@pytest.mark.parametrize("name", list(CASES))
def test_bound_is_sound(name, exact):
    c = CASES[name]
    err, B = _errors(c, exact(name))
    fin = np.isfinite(B)
    worst = (err[fin] / B[fin, None]).max() if fin.any() else 0.0
    print(f"{name}: max |s - s~| / B_ref = {worst:.4f}" + ("" if fin.all() else "  (B not finite for some queries)"))
    assert np.isfinite(err[fin]).all() and worst <= 1.0


def test_parent_tail_is_violated_at_1280(exact):
    """the formula before this suite (last term 2^-140): inside at d = 64 and 1024, violated at d = 1280"""
    for d, broken in ((64, False), (1024, False), (1280, True)):
        name = f"subnormal_scores_d{d}"
        c = CASES[name]
        err, B = _errors(c, exact(name), sr.PARENT_TAIL)
        e0, b0 = err[0, 0] / ULP, B[0] / ULP
        print(f"{name}: |s - s~| = {e0:.2f} ulp, parent's B = {b0:.2f} ulp, now {sr.bound(c.xq[:1], sr.stats(c.xb), sr.pad(d, 32), sr.pad(d, 64))[0] / ULP:.2f} ulp")
        assert e0 == d / 2 and exact(name)[0, 0] == 0.0  # every step a tie
        assert (err > B[:, None]).any() == broken
        if broken:
            assert err[0, 0] > B[0]


def _rho(c, p, s):
    q, v = c.expect["query"], c.expect["victim"]
    o = p["queries"][q]
    return (-float(p["approx"][q, v]) - o["t"]) / (2.0 * o["B"])


def _topk(score, k):
    return set(np.argsort(-score.astype(np.float64), kind="stable")[:k].tolist())


# what the g terms leave of rho when the first (second) term is met exactly: 1 / (1 + d (2^-22 + 2^-24) X' / R) with
# X' / R <= (2^13 + 2 * 64 + 64 * 28) / 3.75 over the d = 1024 case's rows (lo + the largest h of a solid row), minus the
# victim's distance from the edge, at most 2 * 64 of a window of more than 7680
RHO_MIN = {"aligned_rows_d64": 0.9, "aligned_query_d64": 0.9,
           "aligned_rows_d1024": 1.0 / (1.0 + 1024 * (2.0 ** -22 + 2.0 ** -24) * (2 ** 13 + 128 + 64 * 28) / 3.75) - 128.0 / 7680.0}


@pytest.mark.parametrize("name", list(RHO_MIN))
def test_aligned_cases_reach_the_edge(name, exact, pred):
    c, p, s = CASES[name], pred(name), exact(name)
    q, v, k = c.expect["query"], c.expect["victim"], c.k
    top_exact, top_approx = _topk(s[q], k), _topk(p["approx"][q], k)
    rho = _rho(c, p, s)
    print(f"{name}: rho = {rho:.4f} (at least {RHO_MIN[name]:.4f}), window {len(p['queries'][q]['inside'])} rows, candidates_max {p['candidates_max']}")
    assert v in top_exact and v not in top_approx
    assert all(dd in top_approx and dd not in top_exact for dd in c.expect["decoys"][:1])
    assert v in set(p["queries"][q]["inside"].tolist())
    assert RHO_MIN[name] <= rho < 1.0
    # a library whose bound is 10 % short: the window loses the victim (d = 64; at d = 1024 the g terms hide 10 %)
    short = sr.predict(c.xb, c.xq, k, bscale=0.9)
    lost = top_exact - set(short["queries"][q]["inside"].tolist())
    assert (v in lost) == (rho > 0.9)
    if name.endswith("d64"):
        assert lost


@pytest.mark.parametrize("name", ["flushed_fits", "flushed_overflow"])
def test_flushed_rows_score_exactly_zero(name, exact, pred):
    c, p, s = CASES[name], pred(name), exact(name)
    fl = np.array(c.expect["flushed"])
    h, _ = sr.copies(c.xb[fl], -128)
    assert (h[:, 1:] == 0).all() and (h[:, 0] != 0).all() and (np.abs(c.xb[fl, 1:]).max(1) > 0).all()
    assert len(fl) >= c.k
    for q in range(len(c.xq)):
        assert (p["approx"][q, fl] == 0).all()
        assert len(np.unique(s[q, fl])) == len(fl) and (s[q, fl] != 0).all()
        assert (p["approx"][q, np.setdiff1d(np.arange(len(c.xb)), fl)] < 0).all()


@pytest.mark.parametrize("name", list(CASES))
def test_prediction_is_what_the_construction_says_and_robust(name, pred):
    c, p = CASES[name], pred(name)
    kp = sr.kprime(c.k)
    print(f"{name}: fallback {p['fallback']}, candidates_max {p['candidates_max']}, "
          f"windows {[len(o['inside']) for o in p['queries']]}, fits {[o['fits'] for o in p['queries']]}, flagged {[o['flagged'] for o in p['queries']]}")
    if c.expect.get("fallback") is not None:
        assert p["fallback"] == c.expect["fallback"]
    if c.expect.get("candidates_max") is not None:
        assert p["candidates_max"] == c.expect["candidates_max"]
    if p["fallback"] is False:
        assert all(o["fits"] and not o["flagged"] for o in p["queries"])
        assert c.k <= p["candidates_max"] <= kp
        if name.startswith(("aligned", "flushed")):
            assert c.k < p["candidates_max"]  # (the window holds more than the answer)
    if name == "flushed_overflow":
        assert not any(o["fits"] for o in p["queries"])
    if name == "tiny_subnormal_query_d64":
        assert not p["approx"].any() and not p["queries"][0]["fits"]  # (every approximate score is 0)
    if name == "gate_over":
        assert [o["flagged"] for o in p["queries"]] == [False, True, False, True, False]
    if name == "overflowing_norm":
        assert all(o["flagged"] for o in p["queries"])
    sr.assert_robust(p, name)


def test_tiny_answers_need_clamped_rows(exact, pred):
    """only six rows lie above the clamp: every exact top-10 holds rows whose exponent is clamped, every score is below the
    normal range, and every window fits -- the search must deliver the prefilter's own output"""
    c, p, s = CASES["tiny_d64"], pred("tiny_d64"), exact("tiny_d64")
    clamped = np.abs(c.xb).max(1) < 2.0 ** -115
    for q in range(len(c.xq)):
        top = sorted(_topk(s[q], c.k))
        assert clamped[top].sum() >= c.k - 6 and (np.abs(s[q, top]) < 2.0 ** -126).all() and (s[q, top] > 0).all()
        assert clamped[p["queries"][q]["inside"]].sum() >= c.k - 6
    for name in ("subnormal_query_d64", "subnormal_scores_d64_p125"):
        cc, ss = CASES[name], exact(name)
        assert not pred(name)["fallback"]
        best = np.sort(ss, axis=1)[:, -cc.k:]
        assert (best > 0).all() and (best[:, 0] < 2.0 ** -126).all(), name  # (subnormal scores inside every top-k)


def test_add_order_variants_are_robust():
    """the index that once held the victim and was reset: the benign rows' statistics give a smaller window"""
    c = CASES["aligned_rows_d64"]
    a, b = c.parts["special"]
    benign = c.xb[:a]
    p = sr.predict(benign, c.xq, c.k)
    stale = sr.predict(benign, c.xq, c.k, st=sr.stats(c.xb))
    print(f"benign rows: candidates_max {p['candidates_max']}; with the victim's stale statistics {stale['candidates_max']}")
    sr.assert_robust(p, "benign")
    assert not p["fallback"] and p["candidates_max"] == c.k < stale["candidates_max"]


def test_copies_by_hand():
    """the copy format on values typed in by hand: exponent, clamp, flush, zero and non-finite vectors"""
    x = np.zeros((7, 4), np.float32)
    x[0] = [1.0, 2.0 ** -27, 2.0 ** -28 * 1.5, -1.5]            # e = -13; 2^-27 scales to 2^-14 (kept), 1.5 2^-28 to 1.5 2^-15 (flushed)
    x[1] = [2.0 ** -114, 0, 0, 2.0 ** -141]                      # e = -127
    x[2] = [2.0 ** -115, 0, 0, 2.0 ** -142]                      # e = -128
    x[3] = [2.0 ** -116, 2.0 ** -142, 2.0 ** -143, 0]            # clamped at -128: scaled 2^12, 2^-14 (kept), 2^-15 (flushed)
    x[4] = [2.0 ** -149, 0, 0, 0]                                # subnormal: clamped, scaled 2^-21, flushed
    x[6] = [np.inf, 1.0, np.nan, 0]
    h, e = sr.copies(x, -128)
    assert e.tolist() == [-13, -127, -128, -128, -128, 0, 0]
    assert h[0].tolist() == [8192.0, 2.0 ** -14, 0.0, -12288.0]
    assert h[1].tolist() == [8192.0, 0, 0, 2.0 ** -14] and h[2].tolist() == [8192.0, 0, 0, 2.0 ** -14]
    assert h[3].tolist() == [4096.0, 2.0 ** -14, 0, 0] and not h[4].any() and not h[5].any()
    _, eq = sr.copies(x[4:6])
    assert eq.tolist() == [-162, 0]                              # queries are not clamped
    assert sr.kprime(1) == 65 and sr.kprime(64) == 128 and sr.kprime(100) == 200 and sr.kprime(1500) == 2048
