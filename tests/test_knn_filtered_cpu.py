"""Filtered retrieval, the parts that need no device: the C ABI's new symbols against their Python mirror, the mask stride, the host
packer, the per-shard index lists, the script's flag and the refusals the binding makes before anything reaches the library."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rdm_knn_mask_words", "rdm_knn_filtered", "rdm_knn_filtered_f64", "rdm_op_knn_stages_filtered", "rdm_op_row_mask", "rdm_op_row_mask_count")


def _lib():
    import rdm_amd  # noqa: F401
    from rdm_amd import _lib
    return _lib


def test_new_symbols_in_header_and_signatures():
    _lib_ = _lib()
    header = open(os.path.join(ROOT, "include", "rdm_hip.h")).read()
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in rdm_hip.h"
        args = [a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()]
        res, argtypes = _lib_.SIGNATURES[name]
        assert len(argtypes) == len(args), (name, len(argtypes), args)
        assert getattr(_lib_.lib, name).argtypes == argtypes


def test_mask_words_is_n_rounded_up_to_the_tile():
    _lib_ = _lib()
    for base in (64, 256, 4096, 20_927_907):
        for n in range(max(1, base - 2), base + 3):
            assert _lib_.lib.rdm_knn_mask_words(n) == (n + 255) // 256 * 256 // 64 == _lib_.knn_mask_words(n), n
    assert _lib_.knn_mask_words(1) == 4 and _lib_.knn_mask_words(257) == 8 and _lib_.knn_mask_words(0) == 0


def test_pack_row_mask_is_little_endian_packbits():
    _lib_ = _lib()
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 255, 256, 257, 4097):
        a = rng.random(n) < 0.3
        a[-1] = True
        w = _lib_.pack_row_mask(a)
        assert w.dtype == np.int64 and w.shape == (_lib_.knn_mask_words(n),)
        bytes_ = np.packbits(a, bitorder="little")
        assert np.array_equal(w.view(np.uint8)[:len(bytes_)], bytes_) and not w.view(np.uint8)[len(bytes_):].any()
        for r in (0, n // 2, n - 1):
            assert bool((int(w.view(np.uint64)[r // 64]) >> (r % 64)) & 1) == bool(a[r])
    for bad in (np.zeros(4, np.int64), np.zeros((2, 2), bool), np.zeros(0, bool)):
        with pytest.raises(_lib_.RdmError):
            _lib_.pack_row_mask(bad)


def test_shard_row_mask_at_an_odd_row0():
    _lib_ = _lib()
    n, row0, n_local = 1000, 333, 334                     # the middle shard of three; 333 is no multiple of 64
    rows = np.array([0, 332, 333, 334, 400, 400, 666, 667, 999])
    assert _lib_.shard_row_mask(rows, row0, n_local).tolist() == [0, 1, 67, 333]
    member = np.zeros(n, bool)
    member[rows] = True
    assert _lib_.shard_row_mask(member, row0, n_local).tolist() == [0, 1, 67, 333]
    # the shards' local masks together are the global mask
    parts = [(0, 333), (333, 334), (667, 333)]
    back = np.concatenate([np.isin(np.arange(nl), _lib_.shard_row_mask(rows, r0, nl)) for r0, nl in parts])
    assert np.array_equal(back, member)
    assert _lib_.shard_row_mask(np.zeros(0, np.int64), row0, n_local).size == 0
    with pytest.raises(_lib_.RdmError):
        _lib_.shard_row_mask(np.array([0.5]), row0, n_local)
    with pytest.raises(_lib_.RdmError):
        _lib_.shard_row_mask(np.array([-1]), row0, n_local)


def test_rdm_sample_parses_db_subset():
    spec = importlib.util.spec_from_file_location("rdm_sample_filtered", os.path.join(ROOT, "scripts", "rdm_sample.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    opt = mod.parse_args([])
    assert opt.db_subset is None and opt.db_subset_invert is False
    opt = mod.parse_args(["--db_subset", "rows.npy", "--db_subset_invert", "--gpus", "2", "--shard_db"])
    assert str(opt.db_subset) == "rows.npy" and opt.db_subset_invert and opt.shard_db
    acts = {a.option_strings[0]: a for a in mod.build_parser()._actions if a.option_strings}
    assert "[native]" in acts["--db_subset"].help and "[native]" in acts["--db_subset_invert"].help
    with pytest.raises(SystemExit):
        mod.parse_args(["--db_subset_invert"])


def test_filter_arguments_refused_before_the_library():
    _lib_ = _lib()
    words, b = 8, 3
    ok = torch.zeros((2, words), dtype=torch.int64)
    allow, n_masks, ids = _lib_.row_filter_args(ok, [0, 1, 1], b, words)
    assert n_masks == 2 and ids.dtype == np.int32 and ids.tolist() == [0, 1, 1]
    assert _lib_.row_filter_args(ok[0], None, b, words)[:2][1] == 1                       # one mask given flat
    assert _lib_.row_filter_args(None, None, b, words) == (None, 0, None)
    with pytest.raises(_lib_.RdmError, match="mask_of_query needs allow"):
        _lib_.row_filter_args(None, [0, 0, 0], b, words)
    with pytest.raises(_lib_.RdmError, match="int64"):
        _lib_.row_filter_args(ok.to(torch.int32), None, b, words)
    with pytest.raises(_lib_.RdmError, match="int64"):
        _lib_.row_filter_args(np.zeros((2, words), np.int64), None, b, words)
    with pytest.raises(_lib_.RdmError, match=r"\[n_masks, 8\]"):
        _lib_.row_filter_args(ok[:, :-1], None, b, words)
    with pytest.raises(_lib_.RdmError, match="one integer per query"):
        _lib_.row_filter_args(ok, [0, 1], b, words)
    with pytest.raises(_lib_.RdmError, match="one integer per query"):
        _lib_.row_filter_args(ok, [0.0, 1.0, 0.0], b, words)
    with pytest.raises(_lib_.RdmError, match="query 2 names mask 2"):
        _lib_.row_filter_args(ok, [0, 1, 2], b, words)
    with pytest.raises(_lib_.RdmError, match="query 0 names mask -1"):
        _lib_.row_filter_args(ok, [-1, 1, 0], b, words)


def test_subset_bookkeeping_needs_no_device():
    """define_subset before train_searcher keeps the rows (the mask is built with the searcher); bad subsets are refused on the host."""
    import rdm_amd  # noqa: F401
    from rdm_amd.data.retrieval_dataset.dsetbuilder import DatasetBuilder
    pool = {"embedding": np.zeros((100, 64), np.float16), "img_id": np.arange(100), "patch_coords": np.zeros((100, 4), np.int64)}
    db = DatasetBuilder(data_pool=pool)
    member = np.zeros(100, bool)
    member[[3, 5, 99]] = True
    db.define_subset("a", [5, 3, 3, 99]).define_subset("b", member)
    assert db.subsets() == {"a": 3, "b": 3} and db._subsets["a"]["mask"] is None
    assert np.array_equal(db._subsets["a"]["rows"], db._subsets["b"]["rows"])
    for bad in ([100], [-1], np.zeros(99, bool), [0.5], np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            db.define_subset("c", bad)
    assert "c" not in db.subsets()
