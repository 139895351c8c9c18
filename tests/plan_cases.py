"""The scan planner's table: the smallest shapes at which each rule of csrc/plan.h still switches, and what the LAST scan
launch of each search looks like.  Two tests read it: test_plan_cpu.py asks the stand-alone planner (csrc/plan_check.cpp,
no GPU), test_plan_gpu.py asks the library after a real search (last_scan() / last_seed()).

All cases use d = 32.  entry: "host" = IndexFlat.search (synchronous: the statistical seed may run), "dev" =
knn_flat_search_dev on the handle's own stream (synchronous too, but the whole batch reaches the piece cutting in one call),
"stream" = knn_flat_search_dev on a caller's stream (no statistical seed).  approx16: the index multiplies bf16 copies of its
rows, as the coarse entry index of IndexHNSWFlat does (searched on a caller's stream); no exported call makes such an index
or reaches its introspection, so these rows are checked against the stand-alone planner only.

EXPECT maps a case's name to (kernel, query_tile, db_tile, nchunks, grid, seed_stride, stat_rank, sample_rows), as last_scan() /
last_seed() report them.  The literals were NOT produced by csrc/plan.h: they come from the planner as it stood in knn355.hip
(today its host side is flat_search.inc) before it moved (make_plan, the head of search_view, the piece cutting of search_keys_impl, taken verbatim from that commit and
compiled for the host with 256 CUs, the MI355X's count), so both tests compare the planner with its predecessor and not with
itself.

SYM_CASES / SYM_EXPECT: the symmetric self-search behind search_self (plan_self_symmetric, sym_work_table).  can_stream: the
caller gave host arrays and holds the copy stream (knn_flat_search_self from 32 MB of result on); force_qt as in knn_set_tuning.
A value is None where the plain path must serve the search, else (kernel, tile rows, tiles, sample stride, sample rows, rank j,
qcap, k_sample, n_expect, groups, (first item of every group ..., item count), run length of the first group, item count, LDS
bytes, workgroups per launch at most, FNV-1a hash of the work table's (qtile, jt0, jcount) in order), as `plan_check sym`
prints them; last_scan() reports the first group's run length as nchunks and the item count as grid.  Every shape the table
was asked to hold is eligible where it should be: none had to move.

RANGE_CASES / RANGE_EXPECT: one block of a range search (plan_range, range_segcap): (kernel, query_tile, db_tile, nqtiles,
nchunks, tiles_base, tiles_rem, grid, diff, LDS bytes, segcap), as `plan_check range` prints them.

The literals of both tables come from self_search_symmetric (flat_search.inc) and range_make_plan / range_search_impl (range.inc)
as they stood before their decisions moved to csrc/plan.h, taken verbatim from that commit and compiled for the host with
256 CUs."""
from collections import namedtuple

NO_POOL, NO_PAIRS, NO_SEED, EXACT_SEED, NORM_L2 = 2, 4, 8, 16, 32
STAT_SEED, NO_STAT_SEED, NO_SYM, NO_TILE_MIN_SEED = 128, 512, 1024, 2048
NO_Q16, NO_BIG_TILE, BIG_TILE = 131072, 262144, 524288
IP, L2 = 0, 1

Case = namedtuple("Case", "name nb nq k metric flags force_qt force_chunks batch entry approx16")


def _c(nb, nq, k, metric=IP, flags=0, qt=0, chunks=0, batch=0, entry="host", approx16=False):
    name = f"nb{nb}-nq{nq}-k{k}-{'l2' if metric else 'ip'}-f{flags}-qt{qt}-c{chunks}-b{batch}-{entry}{'-bf16' if approx16 else ''}"
    return Case(name, nb, nq, k, metric, flags, qt, chunks, batch, entry, approx16)


CASES = []
# tile width
for _f in (0, NO_Q16):
    CASES += [_c(4096, nq, 10, flags=_f) for nq in (32, 33, 48, 49, 64, 65, 96, 97, 128)]
CASES += [_c(nb, nq, 10, flags=BIG_TILE) for nb in (1024, 1023) for nq in (129, 300)]
# the difference build
CASES += [_c(4096, nq, 10, L2) for nq in (1, 8, 9, 12, 13, 16, 17, 19, 20)]
CASES += [_c(4096, 19, 10, L2, flags=NORM_L2), _c(4096, 5, 10, L2, batch=100)]
# pairs, pool, tile-minimum seed
for _f in (0, NO_PAIRS, NO_TILE_MIN_SEED, NO_SEED):
    CASES += [_c(nb, 8, 10, flags=_f) for nb in (16383, 16384, 1 << 18)]
CASES += [_c(1 << 18, 8, 1000)]
# statistical seed, synchronous entry
CASES += [_c(nb, nq, k) for nb in (8191, 8192, 14433) for nq in (64, 65, 200) for k in (100, 301)]
CASES += [_c(14433, nq, 301, flags=f) for nq in (64, 200) for f in (STAT_SEED, NO_STAT_SEED)]
# pieces
CASES += [_c(1 << 18, nq, 10) for nq in (129, 160, 193, 225, 640)]
CASES += [_c(1 << 18, 640, 10, flags=BIG_TILE)]
CASES += [_c(1 << 15, 100, k, entry=e) for k in (100, 300) for e in ("host", "stream")]
CASES += [_c(4096, nq, 10, entry="dev") for nq in (24576, 24577)]
# forced tile and chunks
CASES += [_c(4096, 49, 10, qt=48), _c(4096, 40, 10, qt=48), _c(4096, 8, 10, chunks=3)]
# bf16 rows: no 48- / 96-query tile, no pairs, no tile-minimum seed, no remainder piece on a tile of its own
CASES += [_c(nb, nq, 10, entry="stream", approx16=True) for nb in (4096, 1 << 18) for nq in (8, 200)]

EXPECT = {
    'nb4096-nq32-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq33-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q48_d256', 48, 256, 16, 16, 0, 0, 0),
    'nb4096-nq48-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q48_d256', 48, 256, 16, 16, 0, 0, 0),
    'nb4096-nq49-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq64-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq65-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 32, 32, 0, 0, 0),
    'nb4096-nq96-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 32, 32, 0, 0, 0),
    'nb4096-nq97-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb4096-nq128-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb4096-nq32-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq33-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq48-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq49-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq64-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq65-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb4096-nq96-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb4096-nq97-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb4096-nq128-k10-ip-f131072-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 32, 32, 0, 0, 0),
    'nb1024-nq129-k10-ip-f524288-qt0-c0-b0-host': ('flat_scan_q256_d256', 256, 256, 4, 4, 0, 0, 0),
    'nb1024-nq300-k10-ip-f524288-qt0-c0-b0-host': ('flat_scan_q256_d256', 256, 256, 4, 8, 0, 0, 0),
    'nb1023-nq129-k10-ip-f524288-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 8, 16, 0, 0, 0),
    'nb1023-nq300-k10-ip-f524288-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 8, 24, 0, 0, 0),
    'nb4096-nq1-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq8-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq9-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq12-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq13-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq16-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq17-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq19-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256_l2diff', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq20-k10-l2-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq19-k10-l2-f32-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq5-k10-l2-f0-qt0-c0-b100-host': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb16383-nq8-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, -4, 0, 0),
    'nb16384-nq8-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, -4, 0, 0),
    'nb262144-nq8-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, -1, 0, 0),
    'nb16383-nq8-k10-ip-f4-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 32, 32, 0, 0, 0),
    'nb16384-nq8-k10-ip-f4-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 32, 32, 0, 0, 0),
    'nb262144-nq8-k10-ip-f4-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, 256, 0, 1024),
    'nb16383-nq8-k10-ip-f2048-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, 0, 0, 0),
    'nb16384-nq8-k10-ip-f2048-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, 0, 0, 0),
    'nb262144-nq8-k10-ip-f2048-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, 128, 0, 2048),
    'nb16383-nq8-k10-ip-f8-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, 0, 0, 0),
    'nb16384-nq8-k10-ip-f8-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 64, 64, 0, 0, 0),
    'nb262144-nq8-k10-ip-f8-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, 0, 0, 0),
    'nb262144-nq8-k1000-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, -4, 0, 0),
    'nb8191-nq64-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 64, 64, 0, 0, 0),
    'nb8191-nq64-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 64, 64, 0, 0, 0),
    'nb8191-nq65-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 64, 64, 0, 0, 0),
    'nb8191-nq65-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 64, 64, 0, 0, 0),
    'nb8191-nq200-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 64, 128, 0, 0, 0),
    'nb8191-nq200-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 64, 128, 0, 0, 0),
    'nb8192-nq64-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 64, 64, 0, 0, 0),
    'nb8192-nq64-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 64, 64, 0, 0, 0),
    'nb8192-nq65-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 64, 64, 32, 19, 256),
    'nb8192-nq65-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 64, 64, 32, 33, 256),
    'nb8192-nq200-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 64, 128, 32, 19, 256),
    'nb8192-nq200-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 64, 128, 32, 33, 256),
    'nb14433-nq64-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 112, 112, -2, 0, 0),
    'nb14433-nq64-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 112, 112, 0, 0, 0),
    'nb14433-nq65-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 112, 112, 32, 19, 452),
    'nb14433-nq65-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 112, 112, 32, 33, 452),
    'nb14433-nq200-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 113, 226, 32, 19, 452),
    'nb14433-nq200-k301-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 113, 226, 32, 33, 452),
    'nb14433-nq64-k301-ip-f128-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 112, 112, 32, 33, 452),
    'nb14433-nq64-k301-ip-f512-qt0-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 112, 112, 0, 0, 0),
    'nb14433-nq200-k301-ip-f128-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 113, 226, 32, 33, 452),
    'nb14433-nq200-k301-ip-f512-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 17, 34, 0, 0, 0),
    'nb262144-nq129-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, -1, 0, 0),
    'nb262144-nq160-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q32_d256', 32, 256, 512, 512, -1, 0, 0),
    'nb262144-nq193-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q96_d128', 96, 128, 512, 512, 128, 0, 2048),
    'nb262144-nq225-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 256, 512, 128, 0, 2048),
    'nb262144-nq640-k10-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 98, 490, 32, 0, 8192),
    'nb262144-nq640-k10-ip-f524288-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 512, 512, 128, 0, 2048),
    'nb32768-nq100-k100-ip-f0-qt0-c0-b0-host': ('flat_scan_q48_d256', 48, 256, 128, 128, -4, 0, 0),
    'nb32768-nq100-k100-ip-f0-qt0-c0-b0-stream': ('flat_scan_q48_d256', 48, 256, 128, 128, -4, 0, 0),
    'nb32768-nq100-k300-ip-f0-qt0-c0-b0-host': ('flat_scan_q128_d128', 128, 128, 256, 256, 32, 34, 1024),
    'nb32768-nq100-k300-ip-f0-qt0-c0-b0-stream': ('flat_scan_q48_d256', 48, 256, 128, 128, -4, 0, 0),
    'nb4096-nq24576-k10-ip-f0-qt0-c0-b0-dev': ('flat_scan_q128_d128', 128, 128, 8, 1536, 0, 0, 0),
    'nb4096-nq24577-k10-ip-f0-qt0-c0-b0-dev': ('flat_scan_q128_d128', 128, 128, 11, 715, 0, 0, 0),
    'nb4096-nq49-k10-ip-f0-qt48-c0-b0-host': ('flat_scan_q64_d128', 64, 128, 32, 32, 0, 0, 0),
    'nb4096-nq40-k10-ip-f0-qt48-c0-b0-host': ('flat_scan_q48_d256', 48, 256, 16, 16, 0, 0, 0),
    'nb4096-nq8-k10-ip-f0-qt0-c3-b0-host': ('flat_scan_q32_d256', 32, 256, 3, 3, 0, 0, 0),
    'nb4096-nq8-k10-ip-f0-qt0-c0-b0-stream-bf16': ('flat_scan_q32_d256', 32, 256, 16, 16, 0, 0, 0),
    'nb4096-nq200-k10-ip-f0-qt0-c0-b0-stream-bf16': ('flat_scan_q128_d128', 128, 128, 32, 64, 0, 0, 0),
    'nb262144-nq8-k10-ip-f0-qt0-c0-b0-stream-bf16': ('flat_scan_q32_d256', 32, 256, 512, 512, 256, 0, 1024),
    'nb262144-nq200-k10-ip-f0-qt0-c0-b0-stream-bf16': ('flat_scan_q128_d128', 128, 128, 256, 512, 128, 0, 2048),
}

SymCase = namedtuple("SymCase", "name n k metric flags force_qt can_stream")


def _s(n, k, metric=IP, flags=0, qt=0, stream=0):
    return SymCase(f"n{n}-k{k}-{'l2' if metric else 'ip'}-f{flags}-qt{qt}-s{stream}", n, k, metric, flags, qt, stream)


SYM_CASES = []
# eligibility edge at 3000 rows
SYM_CASES += [_s(n, 10, m) for n in (2999, 3000) for m in (IP, L2)]
# the register select's limit
SYM_CASES += [_s(4096, 1400), _s(4096, 1401)]
# tuning that forbids the launch (beside the same search without it), the 256-row tile on demand
SYM_CASES += [_s(4096, 10, flags=NO_SYM), _s(4096, 10, flags=NO_STAT_SEED), _s(4096, 10, qt=128), _s(4096, 10), _s(4096, 10, flags=BIG_TILE)]
# sample stride 32 -> 64
SYM_CASES += [_s(131071, 10), _s(131072, 10)]
# one group -> four (32 MB of result, 64 tiles) -> eight (256 MB, 128 tiles), and the same shapes without the copy stream
for _st in (1, 0):
    SYM_CASES += [_s(8192, 341, stream=_st), _s(8192, 342, stream=_st), _s(8064, 400, stream=_st)]
    SYM_CASES += [_s(16384, 1365, stream=_st), _s(16384, 1366, stream=_st), _s(16256, 1400, stream=_st)]

SYM_EXPECT = {
    'n2999-k10-ip-f0-qt0-s0': None,
    'n2999-k10-l2-f0-qt0-s0': None,
    'n3000-k10-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 24, 32, 94, 9, 1856, 10, 385, 1, (0, 300), 1, 300, 78864, 4096, 'fafac78b0058c1e5'),
    'n3000-k10-l2-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 24, 32, 94, 9, 1856, 10, 385, 1, (0, 300), 1, 300, 78864, 4096, 'fafac78b0058c1e5'),
    'n4096-k1400-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 32, 32, 128, 78, 11072, 105, 4994, 1, (0, 272), 2, 272, 78864, 1024, 'c58840daad1fb1a5'),
    'n4096-k1401-ip-f0-qt0-s0': None,
    'n4096-k10-ip-f1024-qt0-s0': None,
    'n4096-k10-ip-f512-qt0-s0': None,
    'n4096-k10-ip-f0-qt128-s0': None,
    'n4096-k10-ip-f524288-qt0-s0': ('flat_scan_q256_d256_sym', 256, 16, 32, 128, 9, 1856, 10, 386, 1, (0, 136), 1, 136, 141328, 1024, 'd135e528e5bc2fa5'),
    'n4096-k10-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 32, 32, 128, 9, 1856, 10, 386, 1, (0, 272), 2, 272, 78864, 4096, 'c58840daad1fb1a5'),
    'n131071-k10-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 1024, 32, 4096, 9, 1856, 10, 386, 1, (0, 21484), 25, 21484, 78864, 4096, '8f874418f0989ed5'),
    'n131072-k10-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 1024, 64, 2048, 7, 2240, 10, 594, 1, (0, 21484), 25, 21484, 78864, 4096, '8f874418f0989ed5'),
    'n8192-k341-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 64, 32, 256, 35, 4800, 51, 1882, 1, (0, 442), 5, 442, 78864, 2048, '2ebcf0dde6c68d01'),
    'n8192-k342-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 64, 32, 256, 35, 4800, 51, 1883, 4, (0, 456, 784, 1176, 1312), 2, 1312, 78864, 2048, 'fc3cbbc9749872a5'),
    'n8064-k400-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 63, 32, 252, 39, 5312, 56, 2122, 1, (0, 1024), 2, 1024, 78864, 2048, '3030c60ccf7a7925'),
    'n16384-k1365-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 128, 32, 512, 86, 11648, 115, 5283, 4, (0, 464, 906, 1306, 1578), 8, 1578, 78864, 1024, '1c3108c19bfb62c1'),
    'n16384-k1366-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 128, 32, 512, 86, 11648, 115, 5285, 8, (0, 488, 912, 1389, 1781, 2237, 2565, 2957, 3093), 4, 3093, 78864, 1024, '3257bdca04721468'),
    'n16256-k1400-ip-f0-qt0-s1': ('flat_scan_q128_d128_sym', 128, 127, 32, 508, 87, 11776, 116, 5369, 4, (0, 509, 951, 1351, 1623), 7, 1623, 78864, 1024, '13a31198a978fb9e'),
    'n8192-k341-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 64, 32, 256, 35, 4800, 51, 1882, 1, (0, 442), 5, 442, 78864, 2048, '2ebcf0dde6c68d01'),
    'n8192-k342-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 64, 32, 256, 35, 4800, 51, 1883, 1, (0, 442), 5, 442, 78864, 2048, '2ebcf0dde6c68d01'),
    'n8064-k400-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 63, 32, 252, 39, 5312, 56, 2122, 1, (0, 1024), 2, 1024, 78864, 2048, '3030c60ccf7a7925'),
    'n16384-k1365-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 128, 32, 512, 86, 11648, 115, 5283, 1, (0, 975), 9, 975, 78864, 1024, 'd210bd3f20760090'),
    'n16384-k1366-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 128, 32, 512, 86, 11648, 115, 5285, 1, (0, 975), 9, 975, 78864, 1024, 'd210bd3f20760090'),
    'n16256-k1400-ip-f0-qt0-s0': ('flat_scan_q128_d128_sym', 128, 127, 32, 508, 87, 11776, 116, 5369, 1, (0, 512), 18, 512, 78864, 1024, '3e4a0dff8c519d45'),
}
RangeCase = namedtuple("RangeCase", "name n nq metric batch")


def _r(n, nq, metric, batch=0):
    return RangeCase(f"n{n}-nq{nq}-{'l2' if metric else 'ip'}-b{batch}", n, nq, metric, batch)


RANGE_CASES = [_r(n, nq, m) for n in (4096, 1 << 18) for m in (L2, IP) for nq in (1, 19, 20, 64, 65)]
RANGE_CASES += [_r(4096, 5, L2, batch=100)]

RANGE_EXPECT = {
    'n4096-nq1-l2-b0': ('range_scan_q32_d256_diff', 32, 256, 1, 16, 1, 0, 16, 1, 74880, 256),
    'n4096-nq19-l2-b0': ('range_scan_q32_d256_diff', 32, 256, 1, 16, 1, 0, 16, 1, 74880, 256),
    'n4096-nq20-l2-b0': ('range_scan_q32_d256', 32, 256, 1, 16, 1, 0, 16, 0, 74880, 256),
    'n4096-nq64-l2-b0': ('range_scan_q32_d256', 32, 256, 2, 16, 1, 0, 32, 0, 74880, 256),
    'n4096-nq65-l2-b0': ('range_scan_q128_d128', 128, 128, 1, 32, 1, 0, 32, 0, 67072, 128),
    'n4096-nq1-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 16, 1, 0, 16, 0, 74880, 256),
    'n4096-nq19-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 16, 1, 0, 16, 0, 74880, 256),
    'n4096-nq20-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 16, 1, 0, 16, 0, 74880, 256),
    'n4096-nq64-ip-b0': ('range_scan_q32_d256', 32, 256, 2, 16, 1, 0, 32, 0, 74880, 256),
    'n4096-nq65-ip-b0': ('range_scan_q128_d128', 128, 128, 1, 32, 1, 0, 32, 0, 67072, 128),
    'n262144-nq1-l2-b0': ('range_scan_q32_d256_diff', 32, 256, 1, 512, 2, 0, 512, 1, 74880, 512),
    'n262144-nq19-l2-b0': ('range_scan_q32_d256_diff', 32, 256, 1, 512, 2, 0, 512, 1, 74880, 512),
    'n262144-nq20-l2-b0': ('range_scan_q32_d256', 32, 256, 1, 512, 2, 0, 512, 0, 74880, 512),
    'n262144-nq64-l2-b0': ('range_scan_q32_d256', 32, 256, 2, 256, 4, 0, 512, 0, 74880, 1024),
    'n262144-nq65-l2-b0': ('range_scan_q128_d128', 128, 128, 1, 512, 4, 0, 512, 0, 67072, 504),
    'n262144-nq1-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 512, 2, 0, 512, 0, 74880, 512),
    'n262144-nq19-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 512, 2, 0, 512, 0, 74880, 512),
    'n262144-nq20-ip-b0': ('range_scan_q32_d256', 32, 256, 1, 512, 2, 0, 512, 0, 74880, 512),
    'n262144-nq64-ip-b0': ('range_scan_q32_d256', 32, 256, 2, 256, 4, 0, 512, 0, 74880, 1024),
    'n262144-nq65-ip-b0': ('range_scan_q128_d128', 128, 128, 1, 512, 4, 0, 512, 0, 67072, 504),
    'n4096-nq5-l2-b100': ('range_scan_q32_d256', 32, 256, 1, 16, 1, 0, 16, 0, 74880, 256),
}
