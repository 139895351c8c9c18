"""Consumers of the (hits, scores) arrays as single GPU passes.

Each function keeps the semantics of the reference's per-row Python loop it replaces:
  remove_self_hit         pfam/proteins.py:85-122
  evaluate_faiss          seqvec_search/main.py:53-82 (AUC1 / TP with one family label per id)
  compute_auc1            pfam/proteins_shared.py:139-157 (sets of homologous proteins)
  compute_is_correct      cath/cath.py:76-84 (C/A/T/H level matrix)
  bootstrap_scores        cath/cath.py:404-438 (the 500 resamples behind the accuracy table's confidence intervals)
  class_accuracies        cath/cath.py:441-458 (make_report_accuracies_table's numbers, before pandas formats them)
  compute_tps_comulative  seqvec_search/tp_cumulative.py:15-34
  assemble                pfam/slices/slices.py:256-291 (protein-level hits from slice hits; also run over the
                          MMseqs2 slice hits, slices.py:312-314)
  auc1_assembled          pfam/slices/slices.py:294-305
  slice_tables            pfam/slices/slices.py:49-80 (families inside each slice, family sizes, has_annotation)
  evaluate_slices         pfam/slices/slices.py:101-142 (evaluate: slice-level is_correct, is_ignore and AUC1)
  compute_correctness_array  pfam/proteins.py:201-207 (per-hit "is this a homologue" matrix)
  precision_recall_curve     pfam/proteins.py:626-648 (mean precision / recall per query over score thresholds)
  bucketed_accuracy          pfam/proteins.py:689-729 (accuracy and its standard error per cosine-similarity bucket)
  accuracy_over_hits         pfam/proteins.py:502-507 (make_accuracy_over_hit: mean fraction of homologues found after j hits)
  recall_per_query           pfam/proteins.py:476-496 (recall over the first 300 hits, per query)
  ranked_precision_recall    pfam/pfam.py:570-583 (the dataset-wide precision-recall curve over every hit, ranked at once)
  ranked_cumulative          cath/cath.py:656-675, 738-771; pfam/pfam.py:166-177, 213-236 (is_correct[argsort(key)].cumsum())
  score_quantiles            pfam/proteins.py:626-648 (numpy.quantile over every score: precision_recall_curve's thresholds)
  combine_hits               pfam/proteins.py:216-240 ("combined": MMseqs2 hits with E < 0.1, filled up with k-NN hits)
  merge_hits                 pfam/proteins.py:340-372 ("both aligned": two lists sorted together, repeated ids dropped)
  compare_hits               pfam/pfam.py:349-370, 602-625 (two lists as sets of ids: "TP Set overlap" and auc1s_optimal)
  pearsonr, spearmanr, correlations, rankdata  cath/cath.py:949-952 (the correlations of cosine scores and E-values)
"""
import math
from collections import Counter, namedtuple
from itertools import groupby
from typing import Dict, Iterable, List, NamedTuple, Optional, Sequence, Set, Tuple

import numpy as np
from numpy import ndarray

from . import _lib


def _hits(h):
    h = np.ascontiguousarray(h, dtype=np.int64)
    if h.ndim != 2:
        raise ValueError("hits must be 2-D")
    return h


def _per_query(a, dtype, nq, name):
    """The library reads nq entries through a raw pointer: a shorter array would be read past its end."""
    a = np.ascontiguousarray(a, dtype)
    if a.shape != (nq,):
        raise ValueError(f"{name} must have shape ({nq},), one entry per row of hits, not {a.shape}")
    return a


def remove_self_hit(hits: ndarray, scores: ndarray, self_ids: ndarray = None) -> Tuple[ndarray, ndarray]:
    """Removes the self hit from every row even when an approximate search did not put it
    first; rows that do not contain their own id lose their last hit instead."""
    hits = _hits(hits)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nq, k = hits.shape
    if scores.shape != hits.shape:
        raise ValueError(f"scores {scores.shape} and hits {hits.shape} must have the same shape")
    if k < 2:
        raise ValueError("remove_self_hit needs k >= 2")
    self_ids = np.arange(nq, dtype=np.int64) if self_ids is None else _per_query(self_ids, np.int64, nq, "self_ids")
    print(f"Fixing {int((hits[:, 0] != self_ids).sum())} misplaced self hits")
    ho = np.empty((nq, k - 1), np.int64)
    so = np.empty((nq, k - 1), np.float32)
    missing = np.empty(nq, np.int32)
    _lib.check(_lib.lib().knn_eval_remove_self_hit(hits.ctypes.data, scores.ctypes.data, nq, k, self_ids.ctypes.data,
                                                   ho.ctypes.data, so.ctypes.data, missing.ctypes.data))
    print(f"There are {int(missing.sum())} missing self hits")
    return ho, so


def label_matches(hits: ndarray, labels_q: ndarray, labels_db: ndarray, want_matrix=True):
    """(is_correct bool [nq,k] or None, leading-run length int32 [nq], match count int32 [nq])"""
    hits = _hits(hits)
    nq, k = hits.shape
    lq = _per_query(labels_q, np.int32, nq, "labels_q")
    ldb = np.ascontiguousarray(labels_db, np.int32)
    if ldb.ndim != 1:
        raise ValueError("labels_db must be 1-D")
    ic = np.empty((nq, k), np.uint8) if want_matrix else None
    lead = np.empty(nq, np.int32)
    tp = np.empty(nq, np.int32)
    _lib.check(_lib.lib().knn_eval_labels(hits.ctypes.data, nq, k, lq.ctypes.data, ldb.ctypes.data, ldb.shape[0],
                                          ic.ctypes.data if want_matrix else None, lead.ctypes.data, tp.ctypes.data))
    return (ic.astype(bool) if want_matrix else None), lead, tp


def _family_codes(data):
    fams = sorted(set(data.ids_to_family.values()))
    code = {f: i for i, f in enumerate(fams)}
    lq = np.asarray([code[data.ids_to_family[i]] for i in data.test_ids], np.int32)
    ldb = np.asarray([code[data.ids_to_family[i]] for i in data.train_ids], np.int32)
    sizes = Counter(data.ids_to_family[i] for i in data.train_ids)
    fam_size = np.asarray([sizes[data.ids_to_family[i]] for i in data.test_ids], np.int64)
    return lq, ldb, fam_size


def evaluate_faiss(data, results: ndarray) -> Tuple[List[float], List[float]]:
    """Same lists as seqvec_search.main.evaluate_faiss (AUC1, TP per query)."""
    lq, ldb, fam_size = _family_codes(data)
    _, lead, tp = label_matches(results, lq, ldb, want_matrix=False)
    return [int(a) / int(s) for a, s in zip(lead, fam_size)], [int(t) / int(s) for t, s in zip(tp, fam_size)]


def compute_tps_comulative(data, results: ndarray) -> ndarray:
    lq, ldb, fam_size = _family_codes(data)
    is_correct, _, _ = label_matches(results, lq, ldb)
    max_tp_expanded = fam_size.repeat(is_correct.shape[1]).reshape(is_correct.shape)
    return (is_correct.cumsum(axis=1) / max_tp_expanded).mean(axis=0)


def compute_auc1(hits: ndarray, homologous_proteins: Dict[str, Set[str]], queries: Sequence[str],
                 target_ids: Sequence[str]) -> ndarray:
    hits = _hits(hits)
    nq, k = hits.shape
    pos = {t: i for i, t in enumerate(target_ids)}
    offsets = np.zeros(nq + 1, np.int64)
    members = []
    sizes = np.empty(nq, np.int64)
    for i in range(nq):
        allc = homologous_proteins[queries[i]]
        sizes[i] = max(len(allc), 1)
        rows = sorted(pos[t] for t in allc if t in pos)
        members.extend(rows)
        offsets[i + 1] = len(members)
    members = np.asarray(members, np.int64)
    lead = np.empty(nq, np.int32)
    tp = np.empty(nq, np.int32)
    _lib.check(_lib.lib().knn_eval_sets(hits.ctypes.data, nq, k, offsets.ctypes.data,
                                        members.ctypes.data if members.size else None, lead.ctypes.data, tp.ctypes.data))
    return lead / sizes


def compute_is_correct(results: ndarray, mapping_array: ndarray, query_rows: ndarray = None) -> ndarray:
    """bool [nq, levels, hits]: does hit j share query q's label at level l (cath: C, A, T, H)."""
    results = _hits(results)
    nq, k = results.shape
    mapping = np.ascontiguousarray(mapping_array)
    if mapping.ndim != 2:
        raise ValueError("mapping_array must be [n, levels]")
    # arbitrary label values -> dense int32 codes per level (equality is all that matters)
    codes = np.empty(mapping.shape, np.int32)
    for l in range(mapping.shape[1]):
        _, codes[:, l] = np.unique(mapping[:, l], return_inverse=True)
    qrows = np.arange(nq, dtype=np.int64) if query_rows is None else _per_query(query_rows, np.int64, nq, "query_rows")
    out = np.empty((nq, mapping.shape[1], k), np.uint8)
    _lib.check(_lib.lib().knn_eval_levels(results.ctypes.data, nq, k, qrows.ctypes.data, codes.ctypes.data,
                                          mapping.shape[0], mapping.shape[1], out.ctypes.data))
    return out.astype(bool)


KNN_BOOTSTRAP_MAX_FAMILIES = 16384  # include/knn355.h


def bootstrap_samples(n: int, replicates: int = 500, seed: int = 42) -> ndarray:
    """int32 [replicates, n]: the reference's resamples (cath/cath.py:405, 409), one rng.choice(n, n) per replicate out of
    numpy.random.default_rng(seed).  Drawn on the host, so that the table's numbers are the reference's."""
    n, replicates = int(n), int(replicates)
    if n < 1 or replicates < 0:
        raise ValueError("bootstrap_samples needs n >= 1 and replicates >= 0")
    rng = np.random.default_rng(seed)
    out = np.empty((replicates, n), np.int32)
    for b in range(replicates):
        out[b] = rng.choice(n, n)
    return out


def bootstrap_replicates(is_correct: ndarray, families: ndarray, sample_ids: ndarray):
    """The replicates of the reference's bootstrap (cath/cath.py:408-419) for one method or many, one GPU pass ->
    (normalized float64, raw float64, correct int64, present int32 [nb]); the first three are [nb] for a 1-D is_correct
    and [nm, nb] for a 2-D one.

    is_correct bool [n] or [nm, n]: the top-1 verdict per evaluable query (per method); families [n]: any labels, the
    superfamily of each of those queries (the reference's mapping_array[is_possible, 0]); sample_ids int [nb, n]: the
    resamples, values in [0, n) (bootstrap_samples).  Per replicate: raw is the mean of the resampled verdicts,
    normalized the mean over the superfamilies present in the resample of each one's share of correct members, correct
    the number of correct samples, present the number of superfamilies.  The normalized sum runs in a fixed order
    (include/knn355.h), so it can differ from numpy's pairwise sum in the last bits; raw is the reference's double."""
    ic = np.asarray(is_correct)
    if ic.ndim not in (1, 2):
        raise ValueError("is_correct must be [n] or [nm, n]")
    one = ic.ndim == 1
    ic = np.ascontiguousarray(np.atleast_2d(ic) != 0).view(np.uint8)
    nm, n = ic.shape
    families = np.asarray(families)
    if families.shape != (n,):
        raise ValueError(f"families must have shape ({n},), one label per column of is_correct, not {families.shape}")
    ids = np.asarray(sample_ids)
    if ids.ndim != 2 or ids.shape[1] != n:
        raise ValueError(f"sample_ids must have shape (replicates, {n}), not {ids.shape}")
    if n < 1:
        raise ValueError("bootstrap_replicates needs one query at least")
    if ids.size and (ids.min() < 0 or ids.max() >= n):
        raise ValueError(f"sample_ids must lie in [0, {n})")
    ids = np.ascontiguousarray(ids, np.int32)
    nb = ids.shape[0]
    names, codes = np.unique(families, return_inverse=True)
    if len(names) > KNN_BOOTSTRAP_MAX_FAMILIES:
        raise ValueError(f"families holds {len(names)} distinct labels, more than {KNN_BOOTSTRAP_MAX_FAMILIES}")
    codes = np.ascontiguousarray(codes.reshape(n), np.int32)
    normalized = np.empty((nm, nb), np.float64)
    raw = np.empty((nm, nb), np.float64)
    correct = np.empty((nm, nb), np.int64)
    present = np.empty(nb, np.int32)
    _lib.check(_lib.lib().knn_eval_bootstrap(ic.ctypes.data, nm, n, codes.ctypes.data, len(names), ids.ctypes.data, nb,
                                             correct.ctypes.data, present.ctypes.data, normalized.ctypes.data, raw.ctypes.data))
    if one:
        return normalized[0], raw[0], correct[0], present
    return normalized, raw, correct, present


def bootstrap_scores(is_correct: ndarray, normalized, families: ndarray, replicates: int = 500, seed: int = 42,
                     sample_ids: ndarray = None):
    """The reference's bootstrap_scores (cath/cath.py:404-438) -> (plus_minus_normalized, plus_minus_raw): the larger
    distance from the point estimate to the 2.5 % and the 97.5 % replicate.

    is_correct bool [n] with normalized a float gives two floats; is_correct [nm, n] with normalized [nm] gives two
    float64 [nm] arrays from one GPU pass.  families [n] takes the place of the reference's global
    mapping_array[is_possible, 0]; sample_ids (default: bootstrap_samples(n, replicates, seed), the reference's stream)
    lets a caller draw the resamples once for several calls."""
    ic = np.asarray(is_correct)
    if ic.ndim not in (1, 2):
        raise ValueError("is_correct must be [n] or [nm, n]")
    one = ic.ndim == 1
    ic = np.atleast_2d(ic) != 0
    x = np.atleast_1d(np.asarray(normalized, np.float64))
    if x.shape != (ic.shape[0],):
        raise ValueError(f"normalized must hold one value per method ({ic.shape[0]}), not shape {x.shape}")
    if sample_ids is None:
        sample_ids = bootstrap_samples(ic.shape[1], replicates, seed)
    boot_normalized, boot_raw, _, _ = bootstrap_replicates(ic, families, sample_ids)
    nb = boot_raw.shape[1]
    if nb < 1:
        raise ValueError("bootstrap_scores needs one replicate at least")
    boot_normalized = np.sort(boot_normalized, axis=1)
    boot_raw = np.sort(boot_raw, axis=1)
    lower, upper = int(nb * 0.025), int(nb * 0.975)
    mean = ic.mean(axis=1)
    plus_minus_normalized = np.maximum(x - boot_normalized[:, lower], boot_normalized[:, upper] - x)
    plus_minus_raw = np.maximum(mean - boot_raw[:, lower], boot_raw[:, upper] - mean)
    if one:
        return float(plus_minus_normalized[0]), float(plus_minus_raw[0])
    return plus_minus_normalized, plus_minus_raw


def class_accuracies(is_correct_all_per_method: Dict[str, ndarray], mapping_array: ndarray, bootstrap: bool = False,
                     replicates: int = 500, seed: int = 42, sample_ids: ndarray = None) -> Dict[str, tuple]:
    """The numbers of the reference's make_report_accuracies_table (cath/cath.py:441-458) before pandas formats them:
    name -> (normalized, raw), or (normalized, raw, normalized_stderr, raw_stderr) with bootstrap=True, ordered by
    normalized, descending (equal values keep the order of the input).

    is_correct_all_per_method maps a method to compute_is_correct's bool [n, levels, hits] (its [:, 0, 0] is read: the
    first hit at level 0) or to that bool [n] column itself; mapping_array is [n, levels], level 0 in column 0.  From
    level 0 (cath.py:94-109): is_possible marks the queries whose level-0 family has more than one member,
    normalization is 1 / family size there and 0 elsewhere, families_count the number of such families.  normalized =
    (is_correct * normalization).sum() / families_count, raw = is_correct[is_possible].mean(), in numpy as the reference.
    With bootstrap=True all methods share one batch of resamples and one GPU pass (bootstrap_scores)."""
    mapping = np.asarray(mapping_array)
    if mapping.ndim != 2:
        raise ValueError("mapping_array must be [n, levels]")
    n = mapping.shape[0]
    names, codes, sizes = np.unique(mapping[:, 0], return_inverse=True, return_counts=True)
    member_sizes = sizes[codes.reshape(n)]
    is_possible = member_sizes > 1
    normalization = 1 / member_sizes
    normalization[~is_possible] = 0
    families_count = int((sizes > 1).sum())
    columns = {}
    for name, is_correct in is_correct_all_per_method.items():
        is_correct = np.asarray(is_correct)
        column = is_correct[:, 0, 0] if is_correct.ndim == 3 else is_correct
        if column.shape != (n,):
            raise ValueError(f"is_correct of {name!r} must have one row per row of mapping_array ({n}), not shape {is_correct.shape}")
        columns[name] = column != 0
    if families_count < 1 and columns:
        raise ValueError("no level-0 family has more than one member: nothing can be evaluated")
    out = {name: ((column * normalization).sum() / families_count, column[is_possible].mean()) for name, column in columns.items()}
    if bootstrap and out:
        possible = np.stack([column[is_possible] for column in columns.values()])
        plus_minus = bootstrap_scores(possible, np.asarray([v[0] for v in out.values()]), mapping[is_possible, 0], replicates, seed,
                                      sample_ids)
        for i, name in enumerate(out):
            out[name] = out[name] + (plus_minus[0][i], plus_minus[1][i])
    return dict(sorted(out.items(), key=lambda item: -item[1][0]))


def assemble_grouping(slice_proteins: Sequence[str], db_proteins: Sequence[str] = None):
    """The integer tables knn_eval_assemble takes, from protein names per slice row.

    -> (group_offsets int64 [ng + 1], protein_names [ng], row_group int32 [nb], self_group int32 [ng], id_to_name)

    Query side: runs of consecutive equal names in slice_proteins are the groups (the reference's groupby,
    pfam/slices/slices.py:261), so a name that comes back after another one opens a second query group.  Database side:
    ids go by NAME, in order of first appearance in db_proteins (default: slice_proteins, the self-search), because the
    reference's `picked` set holds names; id_to_name[i] is the name of id i.  self_group[g] is the database id of query
    group g's name, -1 when the database does not hold it."""
    slice_proteins = list(slice_proteins)
    db_proteins = slice_proteins if db_proteins is None else list(db_proteins)
    name_to_id = {}
    for name in db_proteins:
        name_to_id.setdefault(name, len(name_to_id))
    row_group = np.fromiter((name_to_id[name] for name in db_proteins), np.int32, len(db_proteins))
    protein_names, offsets = [], [0]
    for name, run in groupby(slice_proteins):
        protein_names.append(name)
        offsets.append(offsets[-1] + sum(1 for _ in run))
    self_group = np.fromiter((name_to_id.get(name, -1) for name in protein_names), np.int32, len(protein_names))
    return np.asarray(offsets, np.int64), protein_names, row_group, self_group, list(name_to_id)


def assemble(slices_hits: ndarray, slices_scores: ndarray, slice_proteins: Sequence[str], db_proteins: Sequence[str] = None,
             depth: int = None, k_out: int = None, ascending: bool = False, exclude_self: bool = False,
             want_sources: bool = False):
    """Protein-level hits from the hits of a search over slices (pfam/slices/slices.py:256-291), one GPU pass.

    slice_proteins[r] is the protein of query slice row r, db_proteins[h] the protein of database slice row h (default:
    the same list).  Per query protein: the hits of all its slices, best score first (ascending=True: smallest first,
    for e-values; equal scores in input order), cut at depth (default k, as the reference), walked once ignoring hits
    whose protein was already picked -- and, with exclude_self, the query protein itself -- up to k_out (default k; depth when that is smaller).
    -> (groups int64 [ng, k_out] (ids of assemble_grouping's id_to_name, -1 = unfilled), scores float32 [ng, k_out],
    protein_names [ng]) and, with want_sources, qrow and hit int64 [ng, k_out]: the row of slices_hits and the hit id
    each output came from."""
    hits = _hits(slices_hits)
    scores = np.ascontiguousarray(slices_scores, dtype=np.float32)
    ns, k = hits.shape
    if scores.shape != hits.shape:
        raise ValueError(f"scores {scores.shape} and hits {hits.shape} must have the same shape")
    if len(slice_proteins) != ns:
        raise ValueError(f"slice_proteins must name one protein per row of hits ({ns}), not {len(slice_proteins)}")
    offsets, protein_names, row_group, self_group, _ = assemble_grouping(slice_proteins, db_proteins)
    depth = k if depth is None else int(depth)
    k_out = min(k, depth) if k_out is None else int(k_out)
    ng = len(protein_names)
    groups = np.empty((ng, k_out), np.int64)
    out_scores = np.empty((ng, k_out), np.float32)
    qrow = np.empty((ng, k_out), np.int64) if want_sources else None
    hit = np.empty((ng, k_out), np.int64) if want_sources else None
    _lib.check(_lib.lib().knn_eval_assemble(hits.ctypes.data, scores.ctypes.data, ns, k, offsets.ctypes.data, ng,
                                            row_group.ctypes.data if row_group.size else None, row_group.shape[0],
                                            self_group.ctypes.data if exclude_self else None, depth, k_out, 1 if ascending else 0,
                                            groups.ctypes.data, out_scores.ctypes.data,
                                            qrow.ctypes.data if want_sources else None, hit.ctypes.data if want_sources else None))
    if want_sources:
        return groups, out_scores, protein_names, qrow, hit
    return groups, out_scores, protein_names


def auc1_assembled(groups: ndarray, protein_names: Sequence[str], homologous_proteins: Dict[str, Set[str]],
                   id_to_name: Sequence[str]) -> ndarray:
    """pfam/slices/slices.py:294-305: the leading run of correct proteins of every assembled row over the number of
    homologous proteins (an empty set divides by 1, as compute_auc1 does; the reference would divide by zero).  The run
    is knn_eval_sets' leading-run count over the group ids: its binary search finds no -1 among the (non-negative)
    members, so the padding ends a run like any other miss."""
    groups = _hits(groups)
    ng, k_out = groups.shape
    if len(protein_names) != ng:
        raise ValueError(f"protein_names must name one protein per row of groups ({ng}), not {len(protein_names)}")
    name_to_id = {name: i for i, name in enumerate(id_to_name)}
    offsets = np.zeros(ng + 1, np.int64)
    members = []
    sizes = np.empty(ng, np.int64)
    for g in range(ng):
        allc = homologous_proteins[protein_names[g]]
        sizes[g] = max(len(allc), 1)
        members.extend(sorted(name_to_id[t] for t in allc if t in name_to_id))
        offsets[g + 1] = len(members)
    members = np.asarray(members, np.int64)
    lead = np.empty(ng, np.int32)
    tp = np.empty(ng, np.int32)
    if ng and k_out:
        _lib.check(_lib.lib().knn_eval_sets(groups.ctypes.data, ng, k_out, offsets.ctypes.data,
                                            members.ctypes.data if members.size else None, lead.ctypes.data, tp.ctypes.data))
    return lead / sizes


SliceTables = namedtuple("SliceTables", [
    "slice_protein", "slice_start", "slice_stop",                            # int32 [ns]; protein -1: no domain record
    "domain_offsets", "domain_family", "domain_start", "domain_stop",        # int64 [np + 1], int32 [nd] x 3
    "proteins", "families",                                                  # the name of every protein id / family code
    "match_count", "annotation", "has_annotation", "family_sizes"])          # int32 [ns] x 2, bool [ns], int64 [nfam]


def _slice_host_tables(slices, protein_to_domain):
    """The integer tables knn_eval_slice_annotate and knn_eval_slices take (include/knn355.h), built on the host:
    proteins numbered in order of first appearance among the slices, a protein without an entry in protein_to_domain
    being -1; family codes dense, in sorted order of the names that occur in those proteins' domains; the domains of a
    protein sorted by family code (a stable sort: equal families keep the order of the dict's list)."""
    ns = len(slices)
    slice_protein = np.empty(ns, np.int32)
    slice_start = np.empty(ns, np.int32)
    slice_stop = np.empty(ns, np.int32)
    protein_id, proteins = {}, []
    for s, (protein, (start, stop)) in enumerate(slices):
        pid = protein_id.get(protein)
        if pid is None:
            pid = -1
            if protein in protein_to_domain:
                pid = len(proteins)
                proteins.append(protein)
            protein_id[protein] = pid
        slice_protein[s], slice_start[s], slice_stop[s] = pid, start, stop
    families = sorted({pfam for protein in proteins for pfam, _ in protein_to_domain[protein]})
    code = {f: i for i, f in enumerate(families)}
    offsets = np.zeros(len(proteins) + 1, np.int64)
    fam, start, stop = [], [], []
    for p, protein in enumerate(proteins):
        for pfam, (d0, d1) in sorted(protein_to_domain[protein], key=lambda d: code[d[0]]):
            fam.append(code[pfam])
            start.append(d0)
            stop.append(d1)
        offsets[p + 1] = len(fam)
    return (slice_protein, slice_start, slice_stop, offsets, np.asarray(fam, np.int32), np.asarray(start, np.int32),
            np.asarray(stop, np.int32), proteins, families)


def slice_tables(slices: Sequence[Tuple[str, Tuple[int, int]]], protein_to_domain: Dict[str, List[Tuple[str, Tuple[int, int]]]]) -> SliceTables:
    """pfam/slices/slices.py:49-80 as integer tables and one GPU pass.

    slices is the reference's list of (protein, (start, stop)) (slices.py:33-36), protein_to_domain maps a protein to
    its list of (pfam, (start, stop)).  A protein that protein_to_domain does not hold has no domains (the reference
    raises KeyError).  -> SliceTables: the tables (see _slice_host_tables), `families` (the name of every family code)
    and, from knn_eval_slice_annotate: match_count[s], the number of families with a domain inside slice s;
    annotation[s], that family's code when there is exactly one, else -1; has_annotation, the reference's bool array
    (slices.py:76); family_sizes[code], the number of slices with a domain of that family inside (slices.py:70-74)."""
    sp, s0, s1, offsets, fam, d0, d1, proteins, families = _slice_host_tables(slices, protein_to_domain)
    ns, nfam = len(sp), len(families)
    match_count = np.zeros(ns, np.int32)
    annotation = np.full(ns, -1, np.int32)
    family_sizes = np.zeros(nfam, np.int64)
    _lib.check(_lib.lib().knn_eval_slice_annotate(sp.ctypes.data, s0.ctypes.data, s1.ctypes.data, ns, offsets.ctypes.data,
                                                  fam.ctypes.data if fam.size else None, d0.ctypes.data if fam.size else None,
                                                  d1.ctypes.data if fam.size else None, len(proteins), nfam, match_count.ctypes.data,
                                                  annotation.ctypes.data, family_sizes.ctypes.data if nfam else None))
    return SliceTables(sp, s0, s1, offsets, fam, d0, d1, proteins, families, match_count, annotation, annotation >= 0, family_sizes)


def evaluate_slices(hits: ndarray, tables: SliceTables, query_rows: ndarray = None, ignore_unannotated: bool = False,
                    want_column_counts: bool = False):
    """The reference's evaluate (pfam/slices/slices.py:101-142), one GPU pass -> (is_correct bool [nq, k], is_ignore
    bool [nq, k], auc1s float64 [nq]) and, with want_column_counts, the int64 [k] number of rows whose hit j is correct.

    hits [nq, k] are the hits of the query slices query_rows (default: the annotated slices, numpy.flatnonzero(
    tables.has_annotation), as the reference passes slices_hits[has_annotation]).  A hit is correct when the query's
    family has a domain inside the hit slice, ignored when it has one that merely intersects it or, with
    ignore_unannotated, when the hit slice holds no family at all.  auc1s is the number of correct hits in front of the
    first hit that is neither, over the size of the query's family; a query row without an annotation yields 0.  Two
    cases differ from the loop: a hit of -1 (or any id outside the table) names no slice, where the reference's
    slices_pfams_matching[-1] reads the last one; a protein without a domain record has no domains (slice_tables)."""
    hits = _hits(hits)
    nq, k = hits.shape
    ns = len(tables.slice_protein)
    if query_rows is None:
        query_rows = np.flatnonzero(tables.has_annotation)
    query_rows = np.ascontiguousarray(query_rows, np.int64)
    if query_rows.shape != (nq,):
        raise ValueError(f"query_rows must have shape ({nq},), one slice per row of hits, not {query_rows.shape}")
    if nq and (query_rows.min() < 0 or query_rows.max() >= ns):
        raise ValueError(f"query_rows must lie in [0, {ns})")
    annotation = np.ascontiguousarray(tables.annotation[query_rows], np.int32)
    is_correct = np.zeros((nq, k), np.uint8)
    is_ignore = np.zeros((nq, k), np.uint8)
    lead = np.zeros(nq, np.int32)
    tp = np.zeros(nq, np.int32)
    columns = np.zeros(k, np.int64) if want_column_counts else None
    nd = tables.domain_family.size
    if nq and k:
        _lib.check(_lib.lib().knn_eval_slices(
            hits.ctypes.data, nq, k, annotation.ctypes.data, tables.slice_protein.ctypes.data, tables.slice_start.ctypes.data,
            tables.slice_stop.ctypes.data, ns, tables.domain_offsets.ctypes.data, tables.domain_family.ctypes.data if nd else None,
            tables.domain_start.ctypes.data if nd else None, tables.domain_stop.ctypes.data if nd else None, len(tables.proteins),
            len(tables.families), tables.match_count.ctypes.data, 1 if ignore_unannotated else 0, is_correct.ctypes.data,
            is_ignore.ctypes.data, lead.ctypes.data, tp.ctypes.data, columns.ctypes.data if want_column_counts else None))
    annotated = annotation >= 0
    auc1s = np.zeros(nq, np.float64)
    auc1s[annotated] = lead[annotated] / tables.family_sizes[annotation[annotated]]
    out = (is_correct.astype(bool), is_ignore.astype(bool), auc1s)
    return out + (columns,) if want_column_counts else out


def compute_correctness_array(hits: ndarray, homologous_rows: Sequence[Iterable[int]]) -> ndarray:
    """bool [nq, k]: is hit j of query q one of homologous_rows[q] (pfam/proteins.py:201-207; homologous_rows is the
    reference's homologous_proteins_int: per query an iterable of database rows).  A hit that is in no set, -1 included,
    is False."""
    hits = _hits(hits)
    nq, k = hits.shape
    if len(homologous_rows) != nq:
        raise ValueError(f"homologous_rows must hold one set per row of hits ({nq}), not {len(homologous_rows)}")
    offsets = np.zeros(nq + 1, np.int64)
    members = []
    for i in range(nq):
        members.extend(sorted(set(int(t) for t in homologous_rows[i])))
        offsets[i + 1] = len(members)
    members = np.asarray(members, np.int64)
    out = np.empty((nq, k), np.uint8)
    if nq and k:
        _lib.check(_lib.lib().knn_eval_sets_matrix(hits.ctypes.data, nq, k, offsets.ctypes.data,
                                                   members.ctypes.data if members.size else None, out.ctypes.data))
    return out.astype(bool)


def precision_recall_curve(correct: ndarray, scores: ndarray, correct_totals: ndarray, limit: int = 300, smoothness: int = 300,
                           thresholds: ndarray = None, want_counts: bool = False):
    """The reference's precision-recall sweep (pfam/proteins.py:626-648) as one GPU pass -> (recall, precision,
    thresholds), the tuple the reference stores in plot_data[label]; each is float64 [number of thresholds].

    correct bool / uint8 [nq, k] (compute_correctness_array), scores float32 [nq, k], correct_totals [nq] (the number of
    homologues per query, at least 1); only the first `limit` columns count.  At threshold t a hit is predicted when
    its score > t; precision is the mean over queries of (correct predicted / predicted), 1 for a query with no
    prediction, recall the mean of (correct predicted / total).  The means are sums in a fixed order (blocks of 256
    queries, include/knn355.h), so they can differ from numpy.mean's pairwise sum in the last bits.
    thresholds=None: numpy.quantile(scores[:, :limit], numpy.linspace(0, 1, smoothness + 1)), as the reference; the
    quantiles are host work (numpy; computing them on the device is out of scope here).  Thresholds given in any order are
    sorted for the call and the results put back in the caller's order.  want_counts=True appends (selected, tp, empty)
    int64 arrays: predictions and correct predictions summed over the queries, and queries with no prediction."""
    correct = np.asarray(correct)
    if correct.ndim != 2:
        raise ValueError("correct must be 2-D")
    correct = np.ascontiguousarray(correct != 0 if correct.dtype != np.bool_ else correct).view(np.uint8)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    nq, k = correct.shape
    if scores.shape != correct.shape:
        raise ValueError(f"scores {scores.shape} and correct {correct.shape} must have the same shape")
    if nq < 1:
        raise ValueError("precision_recall_curve needs one query at least")
    limit = int(limit)
    if limit < 1 or limit > k:
        raise ValueError(f"limit must be in [1, k = {k}], not {limit}")
    totals = _per_query(correct_totals, np.int64, nq, "correct_totals")
    if (totals < 1).any():
        raise ValueError("correct_totals must be positive: recall divides by them")
    if thresholds is None:
        thresholds = np.quantile(scores[:, :limit], np.linspace(0, 1, int(smoothness) + 1))
    thresholds = np.array(thresholds, dtype=np.float64)
    if thresholds.ndim != 1 or not 1 <= thresholds.size <= 4096:
        raise ValueError("thresholds must be 1-D with 1 .. 4096 entries")
    if np.isnan(thresholds).any():
        raise ValueError("thresholds must not hold NaN")
    order = np.argsort(thresholds, kind="stable")
    thr = np.ascontiguousarray(thresholds[order])
    nthr = thr.size
    precision = np.empty(nthr, np.float64)
    recall = np.empty(nthr, np.float64)
    counts = [np.empty(nthr, np.int64) for _ in range(3)] if want_counts else [None] * 3
    _lib.check(_lib.lib().knn_eval_pr_curve(correct.ctypes.data, scores.ctypes.data, nq, k, limit, totals.ctypes.data,
                                            thr.ctypes.data, nthr, precision.ctypes.data, recall.ctypes.data,
                                            *(c.ctypes.data if want_counts else None for c in counts)))

    def back(a):
        out = np.empty_like(a)
        out[order] = a
        return out

    if want_counts:
        return back(recall), back(precision), thresholds, tuple(back(c) for c in counts)
    return back(recall), back(precision), thresholds


# ---- accuracy per score bucket, accuracy over hits: knn_eval_bucket_counts, knn_eval_hit_curve (include/knn355.h) ------
class BucketedAccuracy(NamedTuple):
    """bucketed_accuracy's result, one entry per bucket: the edges (lo, hi], the member cells, the correct ones, and their
    mean and standard error of the mean (NaN where there is nothing to divide by)."""
    lo: ndarray
    hi: ndarray
    count: ndarray
    correct: ndarray
    precision: ndarray
    sem: ndarray

    def reference_arrays(self):
        """(precision, sem) of the non-empty buckets only, in order: the two arrays the reference builds by `continue`-ing
        over empty buckets (t5_quantized_precision, t5_quantized_precision_sem)."""
        keep = self.count > 0
        return self.precision[keep], self.sem[keep]


def _correct_bytes(correct, who):
    correct = np.asarray(correct)
    if correct.ndim != 2:
        raise ValueError(f"{who}: correct must be 2-D")
    return np.ascontiguousarray(correct != 0 if correct.dtype != np.bool_ else correct).view(np.uint8)


def _limit(limit, k):
    limit = int(limit)
    if limit < 1 or limit > k:
        raise ValueError(f"limit must be in [1, k = {k}], not {limit}")
    return limit


def bucketed_accuracy(correct: ndarray, scores: ndarray, limit: int = 300, smoothness: int = 300, lo: ndarray = None,
                      hi: ndarray = None) -> BucketedAccuracy:
    """The reference's cosine_bucketed_accuracy loop (pfam/proteins.py:689-729) as one GPU pass -> BucketedAccuracy.

    correct bool / uint8 [nq, k] (compute_correctness_array), scores float32 or float64 [nq, k] (anything else is taken as
    float64); only the first `limit` columns count.  A cell is in bucket b when lo[b] < score <= hi[b], compared in
    double.  By default lo = numpy.linspace(0, 1 - (1 / smoothness), smoothness) and hi = lo + (1 / smoothness), the
    reference's own expressions: neighbouring edges then differ in the last bit here and there, so that a cell can be in
    two buckets or in none, and a score of exactly 1.0 can miss the last bucket -- as in the reference.  Edges of one's own
    are each non-decreasing, free of NaN and lo <= hi, 1 .. 4096 of them.
    precision = correct / count in float64, the bits of the reference's bool.mean(), NaN where count == 0.  sem =
    sqrt(c (n - c) / (n (n - 1))) / sqrt(n) from the two integers, NaN for n < 2: scipy.stats.sem of a boolean array in
    closed form, equal to scipy's pairwise-summed value within a few ulp, not bit for bit."""
    correct = _correct_bytes(correct, "bucketed_accuracy")
    scores = np.asarray(scores)
    scores = np.ascontiguousarray(scores, np.float32 if scores.dtype == np.float32 else np.float64)
    nq, k = correct.shape
    if scores.shape != correct.shape:
        raise ValueError(f"scores {scores.shape} and correct {correct.shape} must have the same shape")
    if nq < 1:
        raise ValueError("bucketed_accuracy needs one query at least")
    limit = _limit(limit, k)
    if lo is None and hi is None:
        lo = np.linspace(0, 1 - (1 / smoothness), smoothness)
        hi = lo + (1 / smoothness)
    elif lo is None or hi is None:
        raise ValueError("give both lo and hi, or neither")
    lo = np.ascontiguousarray(lo, np.float64)
    hi = np.ascontiguousarray(hi, np.float64)
    if lo.ndim != 1 or lo.shape != hi.shape or not 1 <= lo.size <= 4096:
        raise ValueError("lo and hi must be 1-D of one length, with 1 .. 4096 entries")
    if np.isnan(lo).any() or np.isnan(hi).any():
        raise ValueError("edges must not hold NaN")
    if (np.diff(lo) < 0).any() or (np.diff(hi) < 0).any() or (lo > hi).any():
        raise ValueError("lo and hi must each be non-decreasing, with lo <= hi")
    nb = lo.size
    count = np.empty(nb, np.int64)
    right = np.empty(nb, np.int64)
    _lib.check(_lib.lib().knn_eval_bucket_counts(scores.ctypes.data, 1 if scores.dtype == np.float64 else 0, correct.ctypes.data, nq, k,
                                                 limit, lo.ctypes.data, hi.ctypes.data, nb, count.ctypes.data, right.ctypes.data))
    n = count.astype(np.float64)
    c = right.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = c / n
        sem = np.sqrt(c * (n - c) / (n * (n - 1))) / np.sqrt(n)
    precision[count == 0] = np.nan
    sem[count < 2] = np.nan
    return BucketedAccuracy(lo, hi, count, right, precision, sem)


def _hit_curve(correct, correct_totals, limit, who):
    correct = _correct_bytes(correct, who)
    nq, k = correct.shape
    if nq < 1:
        raise ValueError(f"{who} needs one query at least")
    limit = _limit(limit, k)
    totals = _per_query(correct_totals, np.int64, nq, "correct_totals")
    if (totals < 1).any():
        raise ValueError("correct_totals must be positive: the curve divides by them")
    mean = np.empty(limit, np.float64)
    rows = np.empty(nq, np.int64)
    _lib.check(_lib.lib().knn_eval_hit_curve(correct.ctypes.data, nq, k, limit, totals.ctypes.data, mean.ctypes.data, rows.ctypes.data, None))
    return mean, rows, totals


def accuracy_over_hits(correct: ndarray, correct_totals: ndarray, limit: int = 300, want_rows: bool = False):
    """The reference's make_accuracy_over_hit(correct[:, :limit]) (pfam/proteins.py:502-507) -> float64 [limit]: entry j is
    the mean over the queries of (correct hits among the first j + 1) / correct_totals.

    correct bool / uint8 [nq, k], correct_totals [nq], at least 1 each.  The mean is the sum of the quotients in row order
    over nq, the order numpy takes for mean(axis=0) of a 2-D array: for limit >= 2 the result has the bits of the
    reference's expression.  For limit = 1 numpy collapses the array and sums pairwise, so there the last bits can differ;
    the order here stays the row order.  want_rows=True appends the int64 [nq] number of correct hits per query among the
    first `limit` (recall_per_query's numerator)."""
    mean, rows, _ = _hit_curve(correct, correct_totals, limit, "accuracy_over_hits")
    return (mean, rows) if want_rows else mean


def recall_per_query(correct: ndarray, correct_totals: ndarray, limit: int = 300) -> ndarray:
    """correct[:, :limit].sum(axis=1) / correct_totals (pfam/proteins.py:478) -> float64 [nq]: the counts from the device,
    the division numpy's own, so the bits are the reference's.  Its mean and scipy.stats.sem stay with the caller."""
    _, rows, _ = _hit_curve(correct, correct_totals, limit, "recall_per_query")
    return rows / np.asarray(correct_totals)


def last_buckets_ms():
    """Milliseconds by HIP events of this thread's last bucketed_accuracy and last accuracy_over_hits / recall_per_query:
    {"bucket_counts": {upload_ms, kernel_ms, download_ms}, "hit_curve": {...}}."""
    from ctypes import c_float
    a, b = (c_float * 3)(), (c_float * 3)()
    _lib.check(_lib.lib().knn_eval_buckets_last_ms(a, b))
    names = ("upload_ms", "kernel_ms", "download_ms")
    return {"bucket_counts": dict(zip(names, a)), "hit_curve": dict(zip(names, b))}


# ---- one stable order over every hit: knn_eval_rank (include/knn355.h) ------------------------------------------------
RANK_MAX_ELEMENTS = 2 ** 31 - 1


def _rank_arrays(scores, correct, limit, flat_ok, who):
    """-> (scores float32 / float64 [rows, k], correct uint8 [rows, k] or None, limit); 1-D input becomes one column"""
    scores = np.asarray(scores)
    if flat_ok and scores.ndim == 1:
        scores = scores.reshape(-1, 1)
    if scores.ndim != 2:
        raise ValueError(f"{who}: scores must be {'1-D or ' if flat_ok else ''}2-D, not {scores.ndim}-D")
    rows, k = scores.shape
    if rows < 1 or k < 1:
        raise ValueError(f"{who}: scores must hold one value at least, not shape {scores.shape}")
    if correct is not None:
        correct = np.asarray(correct)
        if flat_ok and correct.ndim == 1:
            correct = correct.reshape(-1, 1)
        if correct.shape != scores.shape:
            raise ValueError(f"{who}: correct {correct.shape} and scores {scores.shape} must have the same shape")
    limit = k if limit is None else int(limit)
    if limit < 1 or limit > k:
        raise ValueError(f"{who}: limit must be in [1, k = {k}], not {limit}")
    if rows * limit > RANK_MAX_ELEMENTS:
        raise ValueError(f"{who}: {rows} x {limit} values are more than 2^31 - 1")
    scores = np.ascontiguousarray(scores, np.float32 if scores.dtype == np.float32 else np.float64)
    if correct is not None:
        correct = np.ascontiguousarray(correct != 0 if correct.dtype != np.bool_ else correct).view(np.uint8)
    return scores, correct, limit


def _rank(scores, correct, limit, descending=False, want_order=False, want_cum=False, targets=None, ranks=None):
    """knn_eval_rank on checked arrays -> (order, cum, idx, cum_at, sorted_at), None for what was not asked for"""
    rows, k = scores.shape
    n = rows * limit
    order = np.empty(n, np.int64) if want_order else None
    cum = np.empty(n, np.int64) if want_cum else None
    idx = cum_at = sorted_at = None
    nt = nr = 0
    if targets is not None and len(targets):
        targets = np.ascontiguousarray(targets, np.int64)
        nt = targets.size
        idx, cum_at = np.empty(nt, np.int64), np.empty(nt, np.int64)
    if ranks is not None and len(ranks):
        ranks = np.ascontiguousarray(ranks, np.int64)
        nr = ranks.size
        sorted_at = np.empty(nr, scores.dtype)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    _lib.check(_lib.lib().knn_eval_rank(scores.ctypes.data, 1 if scores.dtype == np.float64 else 0, rows, k, limit, ptr(correct),
                                        1 if descending else 0, ptr(order), ptr(cum), ptr(targets) if nt else None, nt, ptr(idx),
                                        ptr(cum_at), ptr(ranks) if nr else None, nr, ptr(sorted_at)))
    return order, cum, idx, cum_at, sorted_at


def last_rank_info():
    """How this thread's last ranked_precision_recall / ranked_cumulative / score_quantiles ran on the device: passes run
    and skipped, tiles, and milliseconds: the device allocations and the host's packing of the first `limit` columns (host
    clock), then upload, sort, scan and look-ups (HIP events)."""
    from ctypes import byref, c_float, c_int32, c_int64
    run, skipped, tiles, ms = c_int32(), c_int32(), c_int64(), (c_float * 6)()
    _lib.check(_lib.lib().knn_last_rank_info(byref(run), byref(skipped), byref(tiles), ms))
    return {"passes_run": run.value, "passes_skipped": skipped.value, "tiles": tiles.value, "alloc_ms": ms[0], "pack_ms": ms[1],
            "upload_ms": ms[2], "sort_ms": ms[3], "scan_ms": ms[4], "lookup_ms": ms[5]}


def _recall_targets(levels: ndarray, total: int) -> ndarray:
    """int64 per level t: the smallest integer c >= 0 with c / total >= t, tested with the float64 division the
    reference's recall array is made of -- so `first r with C(r) >= c` is numpy.searchsorted(C / total, t)."""
    c = np.maximum(np.ceil(levels * total), 0).astype(np.int64)
    while True:
        down = (c > 0) & ((c - 1) / total >= levels)
        if not down.any():
            break
        c[down] -= 1
    while True:
        up = c / total < levels
        if not up.any():
            break
        c[up] += 1
    return c


def ranked_precision_recall(correct: ndarray, scores: ndarray, total_to_be_found: int, limit: int = None, points: int = 10000,
                            descending: bool = False) -> Tuple[ndarray, ndarray]:
    """The dataset-wide precision-recall curve of pfam/pfam.py:570-583 -> (recall, precision), float64 [points].

    Every hit of scores[:, :limit] (float32 or float64 [nq, k]; limit=None: all k columns) is ranked at once, ascending
    (e-values; descending=True for similarities, the order of numpy.argsort(-scores, kind="stable")); C(r) is the number
    of correct hits (correct bool / uint8 [nq, k]) among the ranks 0 .. r; recall(r) = C(r) / total_to_be_found and
    precision(r) = C(r) / (r + 1).  The curve is read at the first rank whose recall reaches each of
    numpy.linspace(0, 1, points), clipped to the last rank, as the reference's searchsorted and clip do.
    The sort and the running count run on the device (knn_eval_rank); the host turns each level into the integer count
    it asks for and divides, with the reference's own int64 / float64 divisions: the results are its bits.
    Equal scores rank in flat order (row, then column), and NaN ranks last: the reference leaves the order of equal scores
    to numpy's default, unstable, sort; here it is the stable one."""
    scores, correct, limit = _rank_arrays(scores, correct, limit, False, "ranked_precision_recall")
    if correct is None:
        raise ValueError("ranked_precision_recall: correct is required")
    total = int(total_to_be_found)
    if total < 1:
        raise ValueError("ranked_precision_recall: total_to_be_found must be positive: recall divides by it")
    points = int(points)
    if points < 1:
        raise ValueError("ranked_precision_recall: points must be positive")
    n = scores.shape[0] * limit
    targets = _recall_targets(np.linspace(0, 1, points), total)
    _, _, idx, cum_at, _ = _rank(scores, correct, limit, descending, targets=targets)
    idx = np.minimum(idx, n - 1)  # (cum_at is C at the clipped rank already)
    return cum_at / total, cum_at / (idx + 1)


def ranked_cumulative(correct: ndarray, keys: ndarray, descending: bool = False, want_order: bool = False):
    """is_correct[numpy.argsort(key, kind="stable")].cumsum() for 1-D or 2-D input (2-D is flattened row by row), the
    cumulative curves of cath/cath.py:656-675, 738-771 and pfam/pfam.py:166-177, 213-236 -> int64 [N], and the order
    itself (int64 [N], flat positions) behind it when want_order.  descending=True ranks by -key; NaN ranks last either
    way, -0.0 equals +0.0, equal keys keep their flat order."""
    keys, correct, limit = _rank_arrays(keys, correct, None, True, "ranked_cumulative")
    if correct is None:
        raise ValueError("ranked_cumulative: correct is required")
    order, cum, _, _, _ = _rank(keys, correct, limit, descending, want_order=want_order, want_cum=True)
    return (cum, order) if want_order else cum


# ---- statistics over contiguous ranges of the ranked order: knn_eval_windows (include/knn355.h) ------------------------
WINDOWS_MAX_COLUMNS = 32


class RollingMeans(NamedTuple):
    keys: ndarray              # float64 [N - W + 1]: the rolling mean of the ranked keys
    values: ndarray            # float64 [M, N - W + 1]: the rolling mean of every column in the keys' order
    order: Optional[ndarray]   # int64 [N] flat positions in rank order (want_order), else None


class RankedBins(NamedTuple):
    start: ndarray    # int64 [bins]: the ranks [start, stop) of every bin
    stop: ndarray
    counts: ndarray   # int64 [M, bins]: set cells of every column in the bin
    mean: ndarray     # float64 [M, bins]: counts / (stop - start); nan for an empty bin
    stderr: ndarray   # float64 [M, bins]: the standard error of that mean (numpy's std() / sqrt(n)); nan for an empty bin
    key_lo: ndarray   # the keys' type [bins]: the key at rank start (even_bins), or the bin's lower edge (edge_bins)
    key_hi: ndarray   # the key at rank stop, or the bin's upper edge (+inf for the last)


def _window_arrays(keys, values, who):
    """-> (keys float32 / float64 [N], values uint8 [M, N] or None for M = 0)"""
    keys = np.asarray(keys)
    if keys.ndim not in (1, 2):
        raise ValueError(f"{who}: keys must be 1-D or 2-D, not {keys.ndim}-D")
    shape = keys.shape
    if keys.size < 1:
        raise ValueError(f"{who}: keys must hold one value at least, not shape {shape}")
    if keys.size > RANK_MAX_ELEMENTS:
        raise ValueError(f"{who}: {keys.size} keys are more than 2^31 - 1")
    if keys.dtype.kind in "iu":  # lengths: exact in float64 below 2^53
        if int(keys.max()) >= 2 ** 53 or int(keys.min()) <= -2 ** 53:
            raise ValueError(f"{who}: an integer key of magnitude 2^53 or more has no exact float64")
        keys = keys.astype(np.float64)
    elif keys.dtype not in (np.float32, np.float64):
        raise ValueError(f"{who}: keys must be float32, float64 or integers, not {keys.dtype}")
    keys = np.ascontiguousarray(keys).reshape(-1)
    if values is None or (not isinstance(values, ndarray) and len(values) == 0):
        return keys, None
    if isinstance(values, ndarray) and values.ndim == 2 and len(shape) == 1:
        columns = list(values)
    elif isinstance(values, ndarray) and values.ndim == 3 and len(shape) == 2:
        columns = list(values)
    elif isinstance(values, ndarray) and values.ndim == 2 and values.shape[1] == keys.size:  # [M, N] over flattened 2-D keys
        columns = [v.reshape(shape) for v in values]
    elif isinstance(values, ndarray):
        raise ValueError(f"{who}: values {values.shape} must be [M, ...] over keys {shape}")
    else:
        columns = [np.asarray(v) for v in values]
    if len(columns) > WINDOWS_MAX_COLUMNS:
        raise ValueError(f"{who}: {len(columns)} columns are more than {WINDOWS_MAX_COLUMNS}")
    if not columns:
        return keys, None
    out = np.empty((len(columns), keys.size), np.uint8)
    for c, v in enumerate(columns):
        if v.shape != shape:
            raise ValueError(f"{who}: column {c} has shape {v.shape}, the keys {shape}")
        if v.dtype != np.bool_ and v.dtype != np.uint8:
            raise ValueError(f"{who}: column {c} must be bool or uint8, not {v.dtype}")
        out[c] = v.reshape(-1) != 0
    return keys, out


def _windows(keys, values, descending, window=0, want_order=False, starts=None, stops=None, edges=None):
    """knn_eval_windows on checked arrays -> (key_means, value_means, order, start, stop, counts, key_lo, key_hi)"""
    n = keys.size
    m = 0 if values is None else values.shape[0]
    nout = n - window + 1 if window else 0
    key_means = np.empty(nout, np.float64) if window else None
    value_means = np.empty((m, nout), np.float64) if window else None
    order = np.empty(n, np.int64) if want_order else None
    nb = len(edges) if edges is not None else (len(starts) if starts is not None else 0)
    start = stop = counts = key_lo = key_hi = None
    if nb:
        start, stop = np.empty(nb, np.int64), np.empty(nb, np.int64)
        counts = np.zeros((m, nb), np.int64)
        key_lo, key_hi = np.empty(nb, keys.dtype), np.empty(nb, keys.dtype)

    def ptr(a):
        return a.ctypes.data if a is not None and a.size else None

    _lib.check(_lib.lib().knn_eval_windows(keys.ctypes.data, 1 if keys.dtype == np.float64 else 0, n, ptr(values), m, 1 if descending else 0, window,
                                           ptr(key_means), ptr(value_means), ptr(order), ptr(starts), ptr(stops), ptr(edges), nb, ptr(start), ptr(stop),
                                           ptr(counts), ptr(key_lo), ptr(key_hi)))
    return key_means, value_means, order, start, stop, counts, key_lo, key_hi


def last_windows_info():
    """How this thread's last rolling_means / even_bins / edge_bins ran on the device: the staging run of the key's chains,
    blocks per run, runs per block, and milliseconds: the device allocations (host clock), then uploads, sort, the gather
    with the scans, the chains, the columns' means, the bins and the downloads (HIP events)."""
    from ctypes import byref, c_float, c_int64
    run, bpr, rpb, ms = c_int64(), c_int64(), c_int64(), (c_float * 8)()
    _lib.check(_lib.lib().knn_last_windows_info(byref(run), byref(bpr), byref(rpb), ms))
    names = ("alloc_ms", "upload_ms", "sort_ms", "gather_scan_ms", "chains_ms", "means_ms", "bins_ms", "download_ms")
    return {"run": run.value, "blocks_per_run": bpr.value, "runs_per_block": rpb.value, **dict(zip(names, ms))}


def rolling_means(keys: ndarray, values=None, window: int = 1000, descending: bool = False, want_order: bool = False) -> RollingMeans:
    """rolling_mean(x[argsort(key)], window) of seqvec_search/utils.py:103 for the key itself and for up to 32 boolean
    columns at once (pfam/pfam.py:247-253, cath/cath.py:799-813, 913-919) -> RollingMeans(keys, values, order).

    keys float32 / float64 (integers such as lengths are taken as float64), 1-D or 2-D (flattened row by row); values a
    bool / uint8 array [M, ...] or a sequence of M arrays shaped like keys, or None.  The order is ranked_cumulative's:
    stable, -0.0 equals +0.0, NaN last, descending=True the order of numpy.argsort(-keys, kind="stable").
    A column's mean over the window is the correctly rounded count / window.  The key's mean adds each window in a fixed
    order (blocks of `window` ranks, a forward and a backward chain per block: include/knn355.h) without any subtraction:
    an inf or a NaN shows in the windows that hold it and in no other."""
    keys, values = _window_arrays(keys, values, "rolling_means")
    window = int(window)
    if window < 1 or window > keys.size:
        raise ValueError(f"rolling_means: window must be in [1, N = {keys.size}], not {window}")
    key_means, value_means, order, *_ = _windows(keys, values, descending, window=window, want_order=want_order)
    return RollingMeans(key_means, value_means, order)


def _ranked_bins(start, stop, counts, key_lo, key_hi):
    n = (stop - start).astype(np.float64)
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = c / n  # (numpy sums a boolean column exactly: these are the bits of its mean())
        stderr = np.sqrt((c * (1 - mean) * (1 - mean) + (n - c) * mean * mean) / n) / np.sqrt(n)
    return RankedBins(start, stop, counts, mean, stderr, key_lo, key_hi)


def even_bins(keys: ndarray, values, bins: int, descending: bool = False) -> RankedBins:
    """hist_evenly of cath/cath.py:863-875 and pfam/pfam.py:282-297: mean and standard error of boolean columns over
    `bins` equal-count slices of the ranked order.  Slice i is the ranks [N * i // (bins + 1), N * (i + 1) // (bins + 1)),
    the reference's own arithmetic: the last 1 / (bins + 1) of the order is never read.  key_lo and key_hi are the keys
    at ranks start and stop, bits untouched, as the reference's tick labels read them.  An empty slice (bins + 1 > N)
    has count 0 and mean = stderr = nan."""
    keys, values = _window_arrays(keys, values, "even_bins")
    bins = int(bins)
    if bins < 1 or bins > 2 ** 20:
        raise ValueError(f"even_bins: bins must be in [1, 2^20], not {bins}")
    i = np.arange(bins + 1, dtype=np.int64)
    cuts = keys.size * i // (bins + 1)
    starts, stops = np.ascontiguousarray(cuts[:-1]), np.ascontiguousarray(cuts[1:])
    _, _, _, start, stop, counts, key_lo, key_hi = _windows(keys, values, descending, starts=starts, stops=stops)
    return _ranked_bins(start, stop, counts, key_lo, key_hi)


def edge_bins(keys: ndarray, values, edges) -> RankedBins:
    """The length bins of cath/cath.py:831-857: bin i holds the keys with edges[i] <= key < edges[i + 1], the last one
    every key >= edges[-1]; NaN keys fall in no bin.  edges ascending and finite, taken in the keys' type; the order is
    ascending.  key_lo, key_hi = edges[i], edges[i + 1] (+inf for the last)."""
    keys, values = _window_arrays(keys, values, "edge_bins")
    e = np.asarray(edges, np.float64).reshape(-1)
    if e.size < 1 or e.size > 2 ** 20:
        raise ValueError(f"edge_bins: need 1 to 2^20 edges, not {e.size}")
    e = np.ascontiguousarray(e.astype(keys.dtype))
    if not np.isfinite(e).all() or (np.diff(e) < 0).any():
        raise ValueError("edge_bins: edges must be finite and ascending")
    _, _, _, start, stop, counts, _, _ = _windows(keys, values, False, edges=e)
    return _ranked_bins(start, stop, counts, e, np.append(e[1:], np.asarray(np.inf, keys.dtype)))


def _quantile_positions(n: int, q: ndarray):
    """numpy 2.2.6's `linear` method (numpy/lib/_function_base_impl.py: _quantile, _get_indexes, _get_gamma): the two
    ranks around each q and the weight between them.  The position is (n - 1) * q; at or past the last rank both ranks
    are -1, the last one, and the weight is still position - (-1)."""
    virtual = (n - 1) * q
    previous = np.floor(virtual)
    following = previous + 1
    above = virtual >= n - 1
    previous[above] = -1
    following[above] = -1
    previous, following = previous.astype(np.intp), following.astype(np.intp)
    return previous, following, virtual - previous


def _quantile_lerp(a: ndarray, b: ndarray, t: ndarray, last) -> ndarray:
    """numpy 2.2.6's _lerp on the order statistics a, b (in the scores' type) with float64 weights t: the difference is
    taken in the scores' type, a + diff * t in float64 below t = 0.5 and b - diff * (1 - t) from there on; a NaN as the
    last order statistic makes every quantile NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        diff = np.subtract(b, a)
        out = np.asarray(np.add(a, diff * t), np.float64)
        high = t >= 0.5
        out[high] = np.subtract(b, diff * (1 - t), dtype=np.float64)[high]
    if np.isnan(last):
        out[:] = last
    return out


def score_quantiles(scores: ndarray, q: ndarray, limit: int = None) -> ndarray:
    """numpy.quantile(scores[:, :limit], q), the default `linear` method, for float32 or float64 scores (2-D, or 1-D) and
    q in [0, 1] -> float64 [len(q)].  precision_recall_curve's default thresholds are
    score_quantiles(scores, numpy.linspace(0, 1, smoothness + 1), limit).

    The device ranks every score (knn_eval_rank) and returns the two order statistics around each q; the host
    interpolates between them as numpy does.  Bit for bit numpy 2.2.6's result, whose arithmetic this restates
    (_quantile_positions, _quantile_lerp); another numpy may round the position or the interpolation differently."""
    scores, _, limit = _rank_arrays(scores, None, limit, True, "score_quantiles")
    q = np.array(q, dtype=np.float64)
    if q.ndim != 1:
        raise ValueError("score_quantiles: q must be 1-D")
    if q.size and not (np.all(q >= 0) and np.all(q <= 1)):
        raise ValueError("score_quantiles: q must be in [0, 1]")
    if not q.size:
        return np.empty(0, np.float64)
    n = scores.shape[0] * limit
    previous, following, gamma = _quantile_positions(n, q)
    ranks = np.concatenate([previous, following, [-1]]) % n
    _, _, _, _, at = _rank(scores, None, limit, ranks=ranks)
    return _quantile_lerp(at[:q.size], at[q.size:2 * q.size], gamma, at[-1])


# ---- tie-averaged ranks and correlations: knn_eval_rankdata, knn_eval_correlate (include/knn355.h) --------------------
KNN_CORR_PEARSON, KNN_CORR_SPEARMAN = 1, 2  # include/knn355.h


class CorrelationResult(NamedTuple):
    statistic: float
    pvalue: float


def _correlate_arrays(x, y, limit, who):
    """-> (x, y, limit): float32 / float64 [rows, k] each, independently, of one shape, two pairs at least"""
    x, _, lim = _rank_arrays(x, None, limit, True, who)
    if y is not None:
        y, _, _ = _rank_arrays(y, None, limit, True, who)
        if x.shape != y.shape:
            raise ValueError(f"{who}: x {x.shape} and y {y.shape} must have the same shape")
    if x.shape[0] * lim < 2:
        raise ValueError(f"{who}: two values at least are needed")
    return x, y, lim


def _wide_sum(lo, hi) -> int:
    """the Python integer of a 128-bit two's-complement sum returned as two uint64 words"""
    v = int(lo) | (int(hi) << 64)
    return v - (1 << 128) if v >> 127 else v


def _ratio(sab: float, saa: float, sbb: float) -> float:
    """sab / (sqrt(saa) * sqrt(sbb)) clipped to [-1, 1]; NaN for a zero denominator (constant input) and for NaN sums"""
    den = math.sqrt(saa) * math.sqrt(sbb) if saa >= 0 and sbb >= 0 else math.nan
    if den == 0 or den != den or sab != sab:
        return math.nan
    r = sab / den
    return r if r != r else max(-1.0, min(1.0, r))


def correlation_pvalue(kind: str, r: float, n: int) -> float:
    """The two-sided p-value scipy.stats reports beside a statistic r over n pairs.  kind "pearson": the exact
    distribution of r under independence, 2 * betainc(n / 2 - 1, n / 2 - 1, (1 - |r|) / 2) (1.0 for n = 2); kind
    "spearman": Student's t with n - 2 degrees of freedom at r * sqrt((n - 2) / ((r + 1) (1 - r))).  Pure host
    arithmetic through scipy.special, imported here: NaN when scipy is not installed, and for a NaN statistic."""
    if kind not in ("pearson", "spearman"):
        raise ValueError(f"correlation_pvalue: kind must be 'pearson' or 'spearman', not {kind!r}")
    if r != r:
        return math.nan
    try:
        from scipy import special
    except ImportError:
        return math.nan
    if kind == "pearson":
        if n == 2:
            return 1.0
        return float(2 * special.betainc(n / 2 - 1, n / 2 - 1, 0.5 * (1 - abs(r))))
    dof = n - 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = r * np.sqrt(np.clip(np.float64(dof) / np.float64((r + 1.0) * (1.0 - r)), 0, None))
    return float(2 * special.stdtr(dof, -abs(t)))


def pearson_statistic(moments: ndarray) -> float:
    """r from knn_eval_correlate's five numbers (mean_x, mean_y, Sxx, Sxy, Syy): Sxy / (sqrt(Sxx) * sqrt(Syy))"""
    return _ratio(float(moments[3]), float(moments[2]), float(moments[4]))


def spearman_statistic(suu: int, suv: int, svv: int) -> float:
    """rho from the exact integer sums over the doubled, centred ranks: float(Suv) / (sqrt(float(Suu)) * sqrt(float(Svv))).
    Where the integers themselves say |rho| = 1 (Suv^2 = Suu Svv, neither 0: a perfectly monotone relation) the result is
    exactly +-1, which the product of two rounded square roots may miss by an ulp."""
    if suu and svv and suv * suv == suu * svv:
        return 1.0 if suv > 0 else -1.0
    return _ratio(float(suv), float(suu), float(svv))


def _correlate(x, y, limit, what):
    """knn_eval_correlate on checked arrays -> (the five Pearson numbers or None, (Suu, Suv, Svv) or None -- not asked
    for, or a NaN in either array --, N)"""
    rows, k = x.shape
    pear = np.full(5, np.nan) if what & KNN_CORR_PEARSON else None
    words = np.zeros(6, np.uint64) if what & KNN_CORR_SPEARMAN else None
    nan = np.zeros(2, np.int64)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    _lib.check(_lib.lib().knn_eval_correlate(x.ctypes.data, 1 if x.dtype == np.float64 else 0, y.ctypes.data, 1 if y.dtype == np.float64 else 0,
                                             rows, k, limit, what, ptr(pear), ptr(words), nan.ctypes.data))
    sums = None
    if words is not None and not nan.any():
        sums = tuple(_wide_sum(words[2 * q], words[2 * q + 1]) for q in range(3))
    return pear, sums, rows * limit


def _pearson_result(pear, n):
    r = pearson_statistic(pear)
    return CorrelationResult(r, correlation_pvalue("pearson", r, n))


def _spearman_result(sums, n):
    r = spearman_statistic(*sums) if sums is not None else math.nan
    return CorrelationResult(r, correlation_pvalue("spearman", r, n))


def last_correlate_ms():
    """How this thread's last rankdata / pearsonr / spearmanr / correlations ran on the device, in milliseconds: the device
    allocations (host clock), then uploads, the sorts, the ranks (tie runs and scatter), the moments and the downloads (HIP
    events)."""
    from ctypes import c_float
    ms = (c_float * 6)()
    _lib.check(_lib.lib().knn_last_correlate_info(ms))
    return dict(zip(("alloc_ms", "upload_ms", "sort_ms", "ranks_ms", "moments_ms", "download_ms"), ms))


def rankdata(a: ndarray, limit: int = None) -> ndarray:
    """scipy.stats.rankdata(a[:, :limit].ravel(), "average"), bit for bit -> float64 [N]: the 1-based rank of every
    value, ties sharing the mean of their ranks (the ranks behind spearmanr, cath/cath.py:952).

    a is float32 or float64, 2-D [rows, k] (limit=None: all k columns) or 1-D.  The device sorts every value at once
    (knn_eval_rankdata), finds the runs of equal values -- -0.0 equals +0.0, infinities order by value -- and returns
    twice the average rank as an exact integer; the halving here is exact.  With a NaN anywhere every rank is NaN, as
    under scipy's default nan_policy="propagate".
    Not here: the other tie methods, nan_policy="omit" or "raise", axis."""
    from ctypes import byref, c_int32
    a, _, limit = _correlate_arrays(a, None, limit, "rankdata")
    rows, k = a.shape
    rank2 = np.empty(rows * limit, np.int64)
    nan = c_int32(0)
    _lib.check(_lib.lib().knn_eval_rankdata(a.ctypes.data, 1 if a.dtype == np.float64 else 0, rows, k, limit, rank2.ctypes.data, byref(nan)))
    if nan.value:
        return np.full(rows * limit, np.nan)
    return rank2 / 2


def pearsonr(x: ndarray, y: ndarray, limit: int = None) -> CorrelationResult:
    """scipy.stats.pearsonr(x[:, :limit].ravel(), y[:, :limit].ravel()) of cath/cath.py:949-951 (the cosine scores against
    the logged E-values) -> CorrelationResult(statistic, pvalue).

    x and y are float32 or float64, independently, of one shape: 2-D [rows, k] (limit=None: all k columns) or 1-D, two
    pairs at least (ValueError otherwise, as scipy raises).  The device widens to float64, takes the two means and then
    the centred sums Sxx, Sxy, Syy, each in one fixed order that depends on N alone (knn_eval_correlate: the same input
    gives the same bits on every run and every device); statistic = Sxy / (sqrt(Sxx) * sqrt(Syy)), clipped to [-1, 1].
    scipy divides by the norms first and sums in its BLAS's order, so its last bits differ.  The statistic is NaN for a
    constant input and when a NaN or an infinity is present.  The pvalue is correlation_pvalue's: NaN without scipy.
    Not here: `alternative` other than two-sided, `method`, `axis`, confidence intervals."""
    x, y, limit = _correlate_arrays(x, y, limit, "pearsonr")
    pear, _, n = _correlate(x, y, limit, KNN_CORR_PEARSON)
    return _pearson_result(pear, n)


def spearmanr(x: ndarray, y: ndarray, limit: int = None) -> CorrelationResult:
    """scipy.stats.spearmanr(x[:, :limit].ravel(), y[:, :limit].ravel()) of cath/cath.py:952 (the cosine scores against
    the E-values) -> CorrelationResult(statistic, pvalue).

    Arrays as for pearsonr.  The device ranks both arrays (rankdata's ranks) and returns the exact integer sums Suu, Suv,
    Svv over the doubled, centred ranks u = 2 rank_x - (N + 1), v = 2 rank_y - (N + 1); statistic = float(Suv) /
    (sqrt(float(Suu)) * sqrt(float(Svv))) from those Python integers, clipped to [-1, 1]: no floating-point sum at all.
    The statistic is NaN for a constant input and when a NaN is present (nan_policy="propagate"); infinities rank like any
    value.  The pvalue is correlation_pvalue's: NaN without scipy.
    Not here: `alternative` other than two-sided, nan_policy="omit" or "raise", `axis`, the matrix-valued form (x with
    several columns as variables)."""
    x, y, limit = _correlate_arrays(x, y, limit, "spearmanr")
    _, sums, n = _correlate(x, y, limit, KNN_CORR_SPEARMAN)
    return _spearman_result(sums, n)


def correlations(x: ndarray, y: ndarray, limit: int = None) -> Tuple[CorrelationResult, CorrelationResult]:
    """(pearsonr(x, y, limit), spearmanr(x, y, limit)) from one call: each array is uploaded once and sorted once.  Ranks
    do not change under a monotone map, so for cath/cath.py:949-952 one call on (scores_best, logged) gives both of its
    statements: logged is numpy.log of the E-values with the zeros' -inf moved to -1e9, below every other logarithm
    (unless an E-value is +inf: the reference's isinf moves that logarithm to -1e9 as well, which is not monotone)."""
    x, y, limit = _correlate_arrays(x, y, limit, "correlations")
    pear, sums, n = _correlate(x, y, limit, KNN_CORR_PEARSON | KNN_CORR_SPEARMAN)
    return _pearson_result(pear, n), _spearman_result(sums, n)


KNN_FUSE_PREFIX_FILL, KNN_FUSE_SORTED_UNION = 0, 1  # include/knn355.h


def _fuse(hits_a, scores_a, keep_a, hits_b, scores_b, mode, ascending, k_out, want_sources):
    """knn_eval_fuse over checked arrays -> (hits, scores, source or None, filled)"""
    hits_a, hits_b = _hits(hits_a), _hits(hits_b)
    scores_a = np.ascontiguousarray(scores_a, dtype=np.float64)
    scores_b = np.ascontiguousarray(scores_b, dtype=np.float64)
    if scores_a.shape != hits_a.shape or scores_b.shape != hits_b.shape:
        raise ValueError(f"scores {scores_a.shape}, {scores_b.shape} and hits {hits_a.shape}, {hits_b.shape} must have the same shapes")
    if hits_a.shape[0] != hits_b.shape[0]:
        raise ValueError(f"both hit lists must have one row per query, not {hits_a.shape[0]} and {hits_b.shape[0]}")
    (nq, ka), kb = hits_a.shape, hits_b.shape[1]
    k_out = ka if k_out is None else int(k_out)
    if keep_a is not None:
        keep_a = np.ascontiguousarray(keep_a, dtype=np.uint8)
        if keep_a.shape != hits_a.shape:
            raise ValueError(f"keep {keep_a.shape} and hits {hits_a.shape} must have the same shape")
    hits = np.empty((nq, max(k_out, 0)), np.int64)
    scores = np.empty(hits.shape, np.float64)
    source = np.empty(hits.shape, np.int32) if want_sources else None
    filled = np.empty(nq, np.int32)
    _lib.check(_lib.lib().knn_eval_fuse(hits_a.ctypes.data, scores_a.ctypes.data, None if keep_a is None else keep_a.ctypes.data, ka,
                                        hits_b.ctypes.data, scores_b.ctypes.data, kb, nq, mode, 1 if ascending else 0, k_out,
                                        hits.ctypes.data, scores.ctypes.data, source.ctypes.data if want_sources else None,
                                        filled.ctypes.data))
    return hits, scores, source, filled


def merge_hits(hits_a: ndarray, scores_a: ndarray, hits_b: ndarray, scores_b: ndarray, k_out: int = None, ascending: bool = True,
               pad_hit: int = -1, pad_score: float = None, want_sources: bool = False):
    """Two hit lists per query sorted together, every hit id already seen dropped (pfam/proteins.py:340-372), one GPU
    pass -> (hits int64 [nq, k_out], scores float64 [nq, k_out]) and, with want_sources, source int32 [nq, k_out].

    hits_a / scores_a [nq, ka] and hits_b / scores_b [nq, kb]; scores are taken as float64 (e-values: float32 cannot
    order those under 1.4e-45).  Per query the entries of both lists are ordered by score (ascending=True: smallest
    first, as for e-values; equal scores in the order of the concatenated lists, NaN last) and walked once, dropping an
    entry whose id came earlier, up to k_out outputs (default: A's width, as the reference).  An entry with a negative
    id does not exist.  source is the column of numpy.concatenate([hits_a, hits_b], axis=1) an output came from, -1
    for padding.  Unfilled slots hold pad_hit and pad_score (default -1 and +-DBL_MAX, as the flat search pads; the
    reference's call is pad_hit=0, pad_score=10**6, which makes its padding an ordinary hit of id 0)."""
    hits, scores, source, filled = _fuse(hits_a, scores_a, None, hits_b, scores_b, KNN_FUSE_SORTED_UNION, ascending, k_out, want_sources)
    if pad_hit != -1 or pad_score is not None:
        unfilled = np.arange(hits.shape[1])[None, :] >= filled[:, None]
        hits[unfilled] = pad_hit
        if pad_score is not None:
            scores[unfilled] = pad_score
    return (hits, scores, source) if want_sources else (hits, scores)


def combine_hits(hits_a: ndarray, e_values_a: ndarray, hits_b: ndarray, scores_b: ndarray, threshold: float = 0.1, k_out: int = None,
                 short: str = "raise", want_sources: bool = False):
    """The hits of A with an e-value under the threshold, filled up with the hits of B that are not among them
    (pfam/proteins.py:216-240: A is MMseqs2's list, B the k-NN list), one GPU pass -> (hits int64 [nq, k_out], scores
    float64 [nq, k_out]) and, with want_sources, source int32 [nq, k_out] (columns of the concatenated lists).

    An entry of A is kept when e_values_a < threshold, in column order, and its score is -numpy.log(e_values_a +
    10**-200) in float64 (numpy on the host, as the reference computes it); B's entries follow in column order with
    their own scores, except those whose id a kept entry of the row carries.  k_out defaults to A's width.  An entry
    with a negative id does not exist.  A row that cannot be filled raises ValueError, as the reference does;
    short="pad" returns it padded with id -1 and score -DBL_MAX instead.  One case differs: a row that becomes full on
    B's very last entry is a full row here, while the reference's `for ... else` raises there (its loop ends without
    meeting the `break` that a further entry would have triggered)."""
    if short not in ("raise", "pad"):
        raise ValueError("short must be 'raise' or 'pad'")
    e_values_a = np.ascontiguousarray(e_values_a, dtype=np.float64)
    keep = e_values_a < threshold
    with np.errstate(divide="ignore", invalid="ignore"):
        scores_a = -np.log(e_values_a + 10**-200)
    hits, scores, source, filled = _fuse(hits_a, scores_a, keep, hits_b, scores_b, KNN_FUSE_PREFIX_FILL, False, k_out, want_sources)
    if short == "raise" and (filled < hits.shape[1]).any():
        row = int(np.argmax(filled < hits.shape[1]))
        raise ValueError(f"row {row} holds {int(filled[row])} hits, fewer than k_out = {hits.shape[1]}")
    return (hits, scores, source) if want_sources else (hits, scores)


# ---- two hit lists compared as sets of ids: knn_eval_overlap (include/knn355.h) ----------------------------------------
class HitOverlap(NamedTuple):
    """compare_hits' result, int32 [nq, 3] each: per query the sizes of (only A, both, only B) for the true-positive sets
    (tp) and for the ids each list returns before its first wrong hit (lead)."""
    tp: ndarray
    lead: ndarray


def compare_hits(hits_a: ndarray, correct_a: ndarray, hits_b: ndarray, correct_b: ndarray) -> HitOverlap:
    """The set comparisons of pfam/pfam.py between two methods' hit lists, query by query, one GPU pass -> HitOverlap.

    hits_a [nq, ka] with correct_a bool / uint8 [nq, ka] (label_matches, compute_correctness_array: non-zero means "this hit
    is a true positive") and hits_b [nq, kb] with its own correct_b; widths 1 .. 2048.  An entry with a negative id does
    not exist (pad ragged MMseqs2 rows with -1): it is in no set and does not end a leading run.
    tp[q] = (|TA - TB|, |TA & TB|, |TB - TA|) over the sets of distinct flagged ids (pfam.py:349-363, A being MMseqs2's list
    there); an id flagged in one list only is in that set only.  lead[q] is the same split of the distinct ids each list
    holds in front of its first existing entry with a zero flag (pfam.py:605-618): lead.sum(axis=1) is the reference's
    len(knn_hits_set | mmseqs_hits_set).  See tp_overlap_fractions and auc1_optimal.
    The joined walk of pfam.py:629-667 (auc1s_joined) is not part of this: merge_hits(..., k_out=ka + kb,
    want_sources=True) gives the walk's order with repeats dropped, and the leading run of correct ids in it is the count."""
    hits_a, hits_b = _hits(hits_a), _hits(hits_b)
    correct_a, correct_b = _correct_bytes(correct_a, "compare_hits"), _correct_bytes(correct_b, "compare_hits")
    if correct_a.shape != hits_a.shape or correct_b.shape != hits_b.shape:
        raise ValueError(f"correct {correct_a.shape}, {correct_b.shape} and hits {hits_a.shape}, {hits_b.shape} must have the same shapes")
    if hits_a.shape[0] != hits_b.shape[0]:
        raise ValueError(f"both hit lists must have one row per query, not {hits_a.shape[0]} and {hits_b.shape[0]}")
    (nq, ka), kb = hits_a.shape, hits_b.shape[1]
    tp = np.empty((nq, 3), np.int32)
    lead = np.empty((nq, 3), np.int32)
    _lib.check(_lib.lib().knn_eval_overlap(hits_a.ctypes.data, correct_a.ctypes.data, ka, hits_b.ctypes.data, correct_b.ctypes.data, kb,
                                           nq, tp.ctypes.data, lead.ctypes.data))
    return HitOverlap(tp, lead)


def tp_overlap_fractions(overlap: HitOverlap, per_query: int = 10) -> Tuple[float, float, float]:
    """The three numbers of the reference's "TP Set overlap" line (pfam/pfam.py:365-370): the sums of only-A, both and only-B
    true positives over the queries, each divided by per_query * nq (the reference's 10 * len(knn_hits))."""
    tp = np.asarray(overlap.tp)
    only_a, both, only_b = (int(c) for c in tp.sum(axis=0, dtype=np.int64))
    denominator = per_query * len(tp)
    return only_a / denominator, both / denominator, only_b / denominator


def auc1_optimal(overlap: HitOverlap, family_sizes: ndarray) -> ndarray:
    """auc1s_optimal of pfam/pfam.py:602-625 -> float64 [nq]: the AUC1 a perfect merger of the two lists could reach,
    len(LA | LB) / family size.  The counts come from the device, the division is numpy's, one per query."""
    lead = np.asarray(overlap.lead)
    sizes = _per_query(family_sizes, np.int64, len(lead), "family_sizes")
    return lead.sum(axis=1, dtype=np.int64) / sizes


def last_overlap_ms():
    """Milliseconds by HIP events of this thread's last compare_hits: {upload_ms, kernel_ms, download_ms}."""
    from ctypes import c_float
    ms = (c_float * 3)()
    _lib.check(_lib.lib().knn_eval_overlap_last_ms(ms))
    return dict(zip(("upload_ms", "kernel_ms", "download_ms"), ms))
