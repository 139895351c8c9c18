"""The cases of tests/test_hnsw_build_exact_gpu.py, shared with tests/test_hnsw_build_reference.py: the CPU test replays every
one of them to the end with the reference's validity conditions holding at every batch, so no GPU case can turn out
unjudgeable on the GPU machine.  NumPy and tests/hnsw_build_reference.py only.

Every case has n <= 1024, d <= 64 and efConstruction = 1024, so condition (a) holds by construction."""
from collections import namedtuple

import numpy as np

import hnsw_build_reference as ref

EFC = 1024

# calls: rows per add call; max_batch: knn_hnsw_set_walk's batch limit (small, so that a few hundred rows are many batches);
# start: rows of a starting graph the reference builds and the test imports (0: from scratch); device_batches: batches that
# must start with >= 64 linked nodes above level 0 (the device path); groups: pruning groups of (65..96, 97..128) members
# the replay must report at least
Case = namedtuple("Case", "name metric M d calls max_batch seed rank start host_upper device_batches groups env walk")


# (seed, rank) of every case's rows.  rank > 0: clusters of that intrinsic dimension; 0: full-rank clusters around heavy rows;
# < 0: one Gaussian cloud in -rank dimensions.  tests/test_hnsw_build_reference.py replays every case under levels drawn
# by the documented law, with conditions (a)-(c) asserted at every batch; a case without an entry is an error.
PICK = {
    "scratch-ip-M4-1call": (16, 2), "scratch-ip-M4-3call": (6, 3), "scratch-ip-M8-1call": (0, 2), "scratch-ip-M8-3call": (0, 2),
    "scratch-l2-M4-1call": (6, 2), "scratch-l2-M4-3call": (25, 2), "scratch-l2-M8-1call": (0, 2), "scratch-l2-M8-3call": (2, 2),
    "hostwalk-ip": (3, 2), "hostwalk-l2": (29, 2), "hostupper-l2-M4": (19, 1),
    "wide-ip-M16": (0, 2), "wide-l2-M16": (0, 2), "wide-ip-M42": (0, -4), "wide-ip-M63": (4, -4), "wide-l2-M63": (0, 0),
    "onebatch-ip": (28, 2), "onebatch-l2": (6, 2),
    "m2-ip-1call-hostbeam": (0, 2), "m2-ip-3call-hostbeam": (3, 2), "m2-l2-1call-hostbeam": (2, 2), "m2-l2-3call-hostbeam": (3, 2),
}


def _case(name, metric, M, d, calls, max_batch, start=0, host_upper=False, device_batches=0, groups=(0, 0), env=(), walk=""):
    seed, rank = PICK[name]
    return Case(name, metric, M, d, tuple(calls), max_batch, seed, rank, start, host_upper, device_batches, groups, tuple(env), walk)


def _split3(n):
    return (n - 2 * (n // 3), n // 3, n // 3)


# from scratch: M = 4 / 8 at n ~ 400 / 800 keeps the nodes above level 0 (one in M) between 64 and 127 for the last third
# of the build
SCRATCH = [_case(f"scratch-{'ip' if metric == 0 else 'l2'}-M{M}-{pieces}call", metric, M, 32, (n,) if pieces == 1 else _split3(n), mb,
                 device_batches=8)
           for metric in (0, 1) for M, n, mb, pieces in ((4, 400, 12, 1), (4, 400, 12, 3), (8, 799, 16, 1), (8, 800, 16, 3))]
WAYS = {"default": {}, "host_links": {"KNN355_HNSW_HOST_LINKS": "1"}, "host_beam": {"KNN355_HNSW_HOST_BEAM": "1"}}

# d = 20: rows are padded to 32 values (dp != d), the device beam is off and host walkers find every candidate
HOST_WALK = [_case(f"hostwalk-{'ip' if metric == 0 else 'l2'}", metric, 4, 20, (300,), 16) for metric in (0, 1)]

# more than 127 nodes above level 0: only the host walkers' upper-level candidates are pinned (their 127 cut is by Vd)
HOST_UPPER = [_case("hostupper-l2-M4", 1, 4, 32, (640,), 8, host_upper=True, device_batches=8,
                    env=(("KNN355_HNSW_HOST_UPPER", "1"),))]

# wide lists: 2M + 1 = 33 / 85 / 127 members before the first new link -- the selection's 64-, 96- and 128-row builds
WIDE = [_case(f"wide-{'ip' if metric == 0 else 'l2'}-M{M}", metric, M, 48, (40, 200), 16384, start=600, device_batches=8, groups=groups)
        for metric, M, groups in ((0, 16, (0, 0)), (1, 16, (0, 0)), (0, 42, (1, 0)), (0, 63, (0, 1)), (1, 63, (0, 1)))]
# (no wide-l2-M42: no L2 rows were found on which an M = 42 list both runs full and keeps condition (b); the 96-row build of
# the selection therefore prunes under the inner product only, its L2 arithmetic is exercised by the 64- and 128-row builds)

# calls of 1, 31 and 32 rows are one batch each, 33 rows are two: the first call is cut into batches of 16, the small calls
# run under the default limit, where only `max(32, n // 32)` and the rows left bound a batch
ONE_BATCH = [_case(f"onebatch-{'ip' if metric == 0 else 'l2'}", metric, 4, 32, (320, 1, 31, 32, 33), (16, 16384, 16384, 16384, 16384))
             for metric in (0, 1)]

# M = 2: two links per node above level 0.  Such a level is not strongly connected even at eight nodes, so "all nodes of the
# level" is not what a walk finds and condition (b) cannot hold.  The library is pinned where its walk is deterministic on
# exact scores -- the host walkers on every level, KNN355_HNSW_HOST_BEAM=1 -- against the reference's restated walk
# (walk_candidates), which needs no level to be connected.  (Level 0 with its four links does not keep (b) either, so the
# device paths of M = 2 stay under the recall tests.)
M2 = [_case(f"m2-{'ip' if metric == 0 else 'l2'}-{pieces}call-hostbeam", metric, 2, 32, (250,) if pieces == 1 else _split3(250), 4,
            env=(("KNN355_HNSW_HOST_BEAM", "1"),), walk="all") for metric in (0, 1) for pieces in (1, 3)]

ALL = M2 + SCRATCH + HOST_WALK + HOST_UPPER + WIDE + ONE_BATCH


def start_levels(n):
    """hand-set levels of a starting graph: one node in six at level 1 or above, one in a hundred and fifty at level 2"""
    lv = np.zeros(n, np.int32)
    lv[::6] = 1
    lv[::150] = 2
    return lv


def rows(case):
    """all rows of a case, the starting graph's first: clusters of a low intrinsic dimension (`rank` Gaussian coordinates
    mapped into d dimensions, plus a little noise in all of them; unit rows for the inner product).  On such rows the
    selection keeps a neighbour per direction and the built graph stays strongly connected on every level, which full-rank
    Gaussian rows do not give at M = 2 .. 8 (hubs take the slots, some nodes are linked by nobody).  A block of exact
    duplicates lies inside one batch and one across two batches of the last add call (the reference's call_batches)"""
    rng = np.random.default_rng(case.seed)
    n = case.start + sum(case.calls)
    ncl = 6 if case.start else max(4, n // 40)
    if case.rank > 0:
        proj = rng.standard_normal((case.rank, case.d))
        z = rng.standard_normal((ncl, case.rank))[rng.integers(0, ncl, n)] + (0.3 if case.start else 0.5) * rng.standard_normal((n, case.rank))
        x = z @ proj + 0.01 * rng.standard_normal((n, case.d))
        if case.metric == ref.METRIC_INNER_PRODUCT:
            x /= np.linalg.norm(x, axis=1, keepdims=True)
    elif case.rank < 0:
        # one full-rank Gaussian cloud in -rank of the d dimensions: near neighbours are not near each other, the selection
        # keeps most of them, lists run full and keep receiving requests
        x = np.zeros((n, case.d))
        x[:, :-case.rank] = rng.standard_normal((n, -case.rank))
    else:
        # full-rank tight clusters around a few heavy rows: everybody's best neighbour is one of few rows, whose full
        # lists keep receiving requests
        cent = 4.0 * rng.standard_normal((ncl, case.d))
        x = cent[rng.integers(0, ncl, n)] + 0.5 * rng.standard_normal((n, case.d))
        hubs = rng.choice(case.start, 2 * ncl, replace=False)
        x[hubs] = (1.5 if case.metric == 0 else 1.0) * cent[np.arange(2 * ncl) % ncl] + 0.05 * rng.standard_normal((2 * ncl, case.d))
    x = np.ascontiguousarray(x, np.float32)
    batches = duplicate_batches(case)
    if batches:
        inside, early, late = batches
        x[inside[1:4]] = x[inside[0]]      # four equal rows in one batch: equal requests, ordered by `from`
        x[late[:3]] = x[early[:3]]         # three rows equal to rows linked before them
    return x


def duplicate_batches(case):
    """the batches of the last add call that take the planted duplicates: (inside, early, late), or None when the call has
    fewer than three batches of four rows (the small last calls of the one-batch cases)"""
    done = case.start + sum(case.calls[:-1])
    batches = [b for b in ref.call_batches(done, done, case.calls[-1], max_batch(case, len(case.calls) - 1)) if len(b) >= 4]
    return (batches[-1], batches[len(batches) // 2], batches[-2]) if len(batches) >= 3 else None


def draw_levels(case, seed=0):
    """levels by the documented law, P(level >= l) = M ** -l, for the rows of the add calls (CPU validity runs: the GPU
    test takes the library's own draws from the exported graph)"""
    rng = np.random.default_rng(1000 + case.seed + seed)
    u = 1.0 - rng.random(sum(case.calls))
    lv = np.floor(-np.log(u) / np.log(case.M)).astype(np.int32)
    return np.minimum(lv, len(ref.level_table(case.M)) - 2)


def start_graph(case, oracle):
    """-> (x, scores, graph, (tables, entry, max_level) of the starting graph or None): the starting graph of a wide-list
    case is built by the reference itself, with hand-set levels"""
    x = rows(case)
    sc = ref.Scores(x, case.metric, oracle)
    g = ref.Graph(case.M)
    if not case.start:
        return x, sc, g, None
    ref.replay_add(g, sc, 0, start_levels(case.start), EFC, 32)
    return x, sc, g, (ref.tables(g), g.entry, g.max_level)


def max_batch(case, c):
    """the batch limit of add call c (one for all calls, or one per call)"""
    return case.max_batch[c] if isinstance(case.max_batch, tuple) else case.max_batch


class Replay:
    """a case replayed call by call: add(levels of the next call's rows) -> (tables, entry, max_level, reports)"""

    def __init__(self, case, oracle):
        self.case = case
        self.x, self.sc, self.g, self.start = start_graph(case, oracle)
        self.after, self.levels = [], np.zeros(0, np.int32)

    def add(self, levels):
        case, c = self.case, len(self.after)
        assert len(levels) == case.calls[c]
        n0 = case.start + sum(case.calls[:c])
        reports = ref.replay_add(self.g, self.sc, n0, levels, EFC, max_batch(case, c), case.host_upper, case.walk)
        self.levels = np.concatenate([self.levels, np.asarray(levels, np.int32)])
        self.after.append((ref.tables(self.g), self.g.entry, self.g.max_level, reports))
        if len(self.after) == len(case.calls):  # the conditions hold for the final graph too: a search of it reaches every row
            ref.assert_conditions(self.g, EFC, case.host_upper, case.walk)
        return self.after[-1]


def replay(case, oracle, levels):
    """levels: of the rows of all add calls -> (x, starting graph or None, [(tables, entry, max_level, reports) after each
    add call], final graph)"""
    r, n0 = Replay(case, oracle), 0
    for n in case.calls:
        r.add(levels[n0:n0 + n])
        n0 += n
    return r.x, r.start, r.after, r.g


def check_reports(case, after):
    reports = [r for a in after for r in a[3]]
    dev = sum(r["upper"] >= 64 for r in reports)
    assert dev >= case.device_batches, f"{case.name}: {dev} batches start with >= 64 linked nodes above level 0, want {case.device_batches}"
    mid, big = sum(r["groups_65_96"] for r in reports), sum(r["groups_97_128"] for r in reports)
    assert mid >= case.groups[0] and big >= case.groups[1], f"{case.name}: pruning groups of 65..96 / 97..128 members: {mid} / {big}, want {case.groups}"
    if case.host_upper:
        assert max(r["upper"] for r in reports) > 127, f"{case.name}: never more than 127 nodes above level 0"
    return dev, mid, big
