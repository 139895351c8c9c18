"""CPU: the C-ABI library loads and exports every symbol include/knn355.h declares; the
Python boundary mirrors the faiss wrapper's argument checks; no compute happens here."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def _declared_symbols():
    text = (ROOT / "include" / "knn355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(knn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    names = _declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), f"libknn355.so does not export {n}"
    # and the ctypes table covers the header
    assert set(names) <= set(_lib.EXPORTS), set(names) - set(_lib.EXPORTS)


def _header_tuning_flags():
    """name -> value of every KNN_TUNE_* enumerator in include/knn355.h (values: integers, <<, |)."""
    text = (ROOT / "include" / "knn355.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flags = {}
    for body in re.findall(r"enum\s*\{(.*?)\}", text, flags=re.S):
        for item in body.split(","):
            m = re.fullmatch(r"\s*(KNN_TUNE_[A-Z0-9_]+)\s*=\s*([0-9<| ()]+?)\s*", item)
            if m:
                assert m.group(1) not in flags, f"{m.group(1)} defined twice"
                flags[m.group(1)] = eval(m.group(2), {"__builtins__": {}})
            else:
                assert "KNN_TUNE_" not in item, f"unparsed enumerator {item.strip()!r}"
    return flags


def test_tuning_flags_match_the_header():
    """knn_set_tuning's flag names and values in _lib.py are those of the header's enum, in both directions."""
    from knn_for_homology_amd import _lib
    header = _header_tuning_flags()
    assert len(header) >= 19
    python = {n: getattr(_lib, n) for n in dir(_lib) if n.startswith("KNN_TUNE_")}
    assert set(python) == set(header), (set(header) - set(python), set(python) - set(header))
    for name, value in header.items():
        assert python[name] == value, f"{name}: header {value}, _lib.py {python[name]}"


def test_version_and_device_count_need_no_gpu():
    from knn_for_homology_amd import _lib
    L = _lib.lib()
    assert b"knn355" in L.knn_version()
    assert _lib.device_count() >= 0


def test_argument_checks_mirror_faiss():
    from knn_for_homology_amd import faiss
    with pytest.raises(TypeError):
        faiss.normalize_L2(np.zeros((2, 4), np.float64))
    with pytest.raises(ValueError):
        faiss.normalize_L2(np.zeros(8, np.float32))
    with pytest.raises(ValueError):
        faiss.normalize_L2(np.zeros((4, 8), np.float32)[:, ::2])
    with pytest.raises(TypeError):
        faiss.normalize_L2([[1.0, 2.0]])
    assert faiss.METRIC_INNER_PRODUCT == 0 and faiss.METRIC_L2 == 1


def test_no_silent_cpu_fallback():
    """Without a device the compute entry points raise; with one they must work -- either
    way nothing is served from the CPU."""
    from knn_for_homology_amd import _lib, faiss
    if _lib.device_count() == 0:
        with pytest.raises(_lib.Knn355Error, match="no HIP device"):
            faiss.IndexFlat(8, faiss.METRIC_L2)
        with pytest.raises(_lib.Knn355Error, match="no HIP device"):
            faiss.normalize_L2(np.ones((2, 8), np.float32))


def test_product_never_imports_oracle():
    pkg = ROOT / "knn-for-homology_amd"
    for f in pkg.rglob("*.py"):
        assert "oracle" not in f.read_text(), f"{f} mentions the oracle"
    for f in (pkg / "csrc").glob("*"):
        if f.suffix in (".hip", ".cpp", ".h", ".inc"):
            assert "knn_oracle" not in f.read_text().replace("oracle/knn_oracle.c", "")
    # developer tools are not allowed to use it either: only tests/, smoke() and bench.py's cpu_baseline
    for f in (ROOT / "tools").rglob("*.py"):
        assert "oracle" not in f.read_text(), f"{f} mentions the oracle"


def test_entry_points_importable():
    from knn_for_homology_amd.cath.search import search, search_and_save  # noqa: F401
    from knn_for_homology_amd.pfam.proteins_search import main, naturalsize  # noqa: F401
    from knn_for_homology_amd.pfam.search import load_embeddings, search_flat, search_index  # noqa: F401
    from knn_for_homology_amd.pfam.slices.slices_search import main as m2  # noqa: F401
    from knn_for_homology_amd.seqvec_search.main import faiss_search, evaluate_faiss, evaluate  # noqa: F401
    from knn_for_homology_amd.seqvec_search.create_index import main as m3  # noqa: F401
    assert naturalsize(819200128) == "819.2 MB"
    assert naturalsize(512) == "512 Bytes"
