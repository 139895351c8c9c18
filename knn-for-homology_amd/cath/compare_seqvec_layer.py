"""Drop-in for the reference's ``cath/compare_seqvec_layer.py``, without its plot.

Inputs, as in the reference (:18-38): the granularity from the command line (5 by default), ``SeqVec CharCNN.npy``,
``SeqVec LSTM1.npy``, ``SeqVec LSTM2.npy`` and ``ids.json`` in the CATH data directory, and the C/A/T/H numbers of every
domain from ``cath-domain-list.txt`` there (the reference caches that table in ``cath-mapping.h5`` through pandas; here the
list file is read directly).  Output (:87-97): ``seqvec_layer.npz`` in the figure directory with
``mean_correct_combinations``, float64 ``[G, 4]``: the three ratios and ``is_correct[:, 3, 0].mean()`` of the mix.

The reference mixes on the host, forks two workers that search one mix each and walks the hits in Python.  Here the three
layers go up once and ``LayerMix.sweep`` returns the counts (layers.py).
"""
import json
import sys
from pathlib import Path
from typing import Optional, Tuple

import numpy
from numpy import ndarray

from ..layers import LayerMix, simplex_ratios
from ..paths import cath_data as _default_cath_data, project_root

LAYER_FILES = ("SeqVec CharCNN.npy", "SeqVec LSTM1.npy", "SeqVec LSTM2.npy")
LEVEL = 3  # the column of mapping_array the reference averages (cath/compare_seqvec_layer.py:89)


def figures() -> Path:
    return project_root() / "more_sensitive" / "cath-figures"


def read_ids(data_dir: Path) -> ndarray:
    """the domain names of ids.json: the third field of each header, up to the slash"""
    headers = json.loads((data_dir / "ids.json").read_text())
    return numpy.asarray([h.split("|")[2].split("/")[0] for h in headers])


def load_mapping(ids, data_dir: Path) -> Tuple[dict, ndarray]:
    """(domain -> its four labels, str array [len(ids), 4]) in the reference's order of levels (cath/cath_shared.py:89-100):
    "C.A.T.H", "C.A.T", "C.A", "C".  Read from the CATH list file: '#' starts a comment, the columns are separated by blanks,
    the first five are the domain name and its C, A, T and H numbers."""
    wanted = set(ids)
    levels = {}
    with open(data_dir / "cath-domain-list.txt") as f:
        for line in f:
            if line.startswith("#"):
                continue
            fields = line.split()
            if len(fields) >= 5 and fields[0] in wanted:
                numbers = [str(int(v)) for v in fields[1:5]]
                levels[fields[0]] = tuple(".".join(numbers[:4 - i]) for i in range(4))
    return levels, numpy.asarray([levels[i] for i in ids])


def mean_correct_combinations(layers, mapping_array: ndarray, granularity: int = 5) -> ndarray:
    """float64 [G, 4]: per grid point its three ratios and the mean top-1 correctness at LEVEL"""
    ratios = simplex_ratios(granularity)
    # (one hit, not cath.search.search's ten: the search is exact and ordered by (score, id), so the first hit is the same)
    swept = LayerMix(layers).sweep(ratios, mapping_array, hits=1, level=LEVEL)
    return numpy.concatenate([ratios, swept.means[:, None]], axis=1)


def main(granularity: int = 5, cath_data: Optional[Path] = None, figure_dir: Optional[Path] = None) -> ndarray:
    data_dir = Path(cath_data) if cath_data is not None else _default_cath_data()
    out_dir = Path(figure_dir) if figure_dir is not None else figures()
    layers = [numpy.load(data_dir / name).astype(numpy.float32, copy=False) for name in LAYER_FILES]
    _, mapping_array = load_mapping(read_ids(data_dir), data_dir)
    print("Mixing, searching and checking hits for correctness")
    result = mean_correct_combinations(layers, mapping_array, granularity)
    out_dir.mkdir(parents=True, exist_ok=True)
    numpy.savez(out_dir / "seqvec_layer.npz", mean_correct_combinations=result)
    return result


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) == 2 else 5)
