"""Host restatement of the ranked consumers (knn_eval_rank in include/knn355.h; evaluation.ranked_precision_recall,
ranked_cumulative, score_quantiles): numpy with kind="stable" after the contract's canonicalisation, the target and clip
arithmetic of the dataset-wide precision-recall curve, and numpy's linear quantile interpolation, one q at a time.
test_rank_reference.py checks this file against the reference's own output (tests/golden/reference_rank.npz) and
against numpy.quantile; test_rank_gpu.py checks the device against this file, bit for bit."""
import numpy as np


def sort_key(scores, descending=False):
    """The array whose numpy.argsort(kind="stable") is the contract's order: -0.0 becomes +0.0 (numpy compares them
    equal anyway); descending negates, which leaves NaN a NaN, and numpy sorts every NaN last, in input order."""
    a = np.array(scores, copy=True)
    a[a == 0] = 0
    return -a if descending else a


def order(scores, limit=None, descending=False):
    """int64 [N]: flat positions p = row * limit + column of scores[:, :limit] in rank order"""
    scores = np.asarray(scores)
    flat = scores.reshape(-1) if scores.ndim == 1 else scores[:, :limit].reshape(-1)
    return np.argsort(sort_key(flat, descending), kind="stable").astype(np.int64)


def flat_correct(correct, limit=None):
    correct = np.asarray(correct)
    flat = correct.reshape(-1) if correct.ndim == 1 else correct[:, :limit].reshape(-1)
    return flat != 0


def cumulative(correct, scores, limit=None, descending=False):
    """-> (C int64 [N], order int64 [N])"""
    o = order(scores, limit, descending)
    return np.cumsum(flat_correct(correct, limit)[o]).astype(np.int64), o


def lookup(C, targets):
    """-> (idx, cum_at): the first r with C[r] >= target (0 for a target <= 0, N for one never reached), and C at
    min(idx, N - 1)"""
    targets = np.asarray(targets, np.int64)
    idx = np.where(targets <= 0, 0, np.searchsorted(C, targets, side="left")).astype(np.int64)
    return idx, C[np.minimum(idx, len(C) - 1)]


def recall_targets(levels, total):
    """per level t the smallest integer c in [0, total] with c / total >= t (float64 division), by search in the table of
    every such quotient"""
    return np.searchsorted(np.arange(total + 1) / total, levels, side="left").astype(np.int64)


def precision_recall_direct(correct, scores, total, limit=None, points=10000, descending=False):
    """The dataset-wide curve of pfam/pfam.py:570-583 straight from its definition, on the stable order: recall(r) =
    C(r) / total and precision(r) = C(r) / (r + 1) as float64 arrays over every rank, read at the first rank whose recall
    reaches each level, or at the last rank when none does -> (recall, precision)"""
    C, _ = cumulative(correct, scores, limit, descending)
    levels = np.linspace(0, 1, points)
    recall_at_rank = C / total
    precision_at_rank = C / (np.arange(len(C)) + 1)
    first = np.minimum(np.searchsorted(recall_at_rank, levels, side="left"), len(C) - 1)
    return recall_at_rank[first], precision_at_rank[first]


def precision_recall(correct, scores, total, limit=None, points=10000, descending=False):
    """the same curve through integer targets, the way the device path takes: level -> count asked for -> first rank that
    has it -> clip -> the two divisions"""
    C, _ = cumulative(correct, scores, limit, descending)
    idx, cum_at = lookup(C, recall_targets(np.linspace(0, 1, points), total))
    idx = np.minimum(idx, len(C) - 1)
    return cum_at / total, cum_at / (idx + 1)


def sorted_scores(scores, limit=None):
    """the scores in rank order, bits untouched"""
    scores = np.asarray(scores)
    flat = scores.reshape(-1) if scores.ndim == 1 else scores[:, :limit].reshape(-1)
    return flat[order(scores, limit)]


def quantiles(scores, q, limit=None):
    """numpy.quantile(scores[:, :limit], q), linear method, as numpy 2.2.6 computes it, one q at a time in Python floats:
    position (n - 1) * q; at or past the last rank both neighbours are the last value and the weight is position + 1; the
    difference of the neighbours in the scores' type; a + diff * t below t = 0.5, b - diff * (1 - t) from there on; all
    NaN when the last value is NaN"""
    s = sorted_scores(scores, limit)
    n = s.size
    out = np.empty(len(q), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j, qq in enumerate(np.asarray(q, np.float64)):
            pos = (n - 1) * float(qq)
            if pos >= n - 1:
                lo = hi = n - 1
                t = pos + 1.0
            else:
                lo = int(np.floor(pos))
                hi = lo + 1
                t = pos - lo
            a, b = s[lo], s[hi]
            diff = np.float64(b - a)  # (the subtraction itself in the scores' type)
            out[j] = np.float64(b) - diff * (1 - t) if t >= 0.5 else np.float64(a) + diff * t
    if np.isnan(s[-1]):
        out[:] = s[-1]
    return out


def bits(a):
    """an array's bits as unsigned integers: equality of these is equality bit for bit, -0.0 and NaN payloads included"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
