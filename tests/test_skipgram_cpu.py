"""srw_skipgram_windows / Engine.skipgram / Engine.walk_skipgram — what can be checked without a GPU: the symbol, its declaration, the
build list, the argument checks that come before the library (or before a device) is touched, and the numpy restatement's own
footing: its Philox against the oracle's, its index map at the ends of the word range.  The batches themselves:
tests/test_gpu_skipgram.py."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import skipgram_ref as ref
from conftest import ROOT
from helpers import pkg


def test_the_library_exports_the_entry_point():
    P = pkg()
    L = P.lib()
    assert "srw_skipgram_windows" in P.EXPORTS and hasattr(L, "srw_skipgram_windows")


def test_the_header_declares_the_struct_and_the_function():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "stellar_rw.h")).read())
    assert "typedef struct { int32_t context; int32_t num_negatives; uint32_t seed; uint32_t epoch; } srw_skipgram_params;" in flat
    assert ("int32_t srw_skipgram_windows(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride, "
            "const srw_skipgram_params *sp, void *d_pos, void *d_neg, int64_t cap_windows, int64_t *n_windows);") in flat
    assert "not filtered" in flat.lower()                     # the header says that negatives may repeat the window's vertices


def test_the_kernel_is_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bskipgram\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert "k_skipgram_fill" in open(os.path.join(csrc, "skipgram.hip")).read()
    assert "skipgram_windows(" in open(os.path.join(csrc, "engine.h")).read()


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of NULL h / sp / n_windows, which comes
    before the handle is looked at.  The checks behind a handle: tests/test_gpu_skipgram.py."""
    import ctypes as C
    P = pkg()
    L = P.lib()
    sp, w = P.SkipgramParams(2, 0, 1, 0), C.c_int64(-7)
    assert L.srw_skipgram_windows(None, None, None, 0, 0, C.byref(sp), None, None, 0, C.byref(w)) == P.ERR_INVALID
    assert L.srw_skipgram_windows(None, None, None, 0, 0, None, None, None, 0, None) == P.ERR_INVALID
    assert w.value == -7
    assert [f[0] for f in P.SkipgramParams._fields_] == ["context", "num_negatives", "seed", "epoch"]
    assert C.sizeof(P.SkipgramParams) == 16


def test_engine_methods_have_the_agreed_parameters():
    P = pkg()
    sig = inspect.signature(P.Engine.skipgram)
    assert list(sig.parameters) == ["self", "context", "num_negatives", "seed", "epoch", "paths", "lens"]
    assert [sig.parameters[k].default for k in ("num_negatives", "seed", "epoch", "paths", "lens")] == [0, 1, 0, None, None]
    sig = inspect.signature(P.Engine.walk_skipgram)
    assert list(sig.parameters) == ["self", "sources", "context", "num_negatives", "sg_seed", "epoch", "walk_kw"]
    assert [sig.parameters[k].default for k in ("num_negatives", "sg_seed", "epoch")] == [0, 1, 0]
    assert sig.parameters["walk_kw"].kind is inspect.Parameter.VAR_KEYWORD


def test_tensor_arguments_are_refused_before_the_library_is_called():
    """An Engine without a handle: anything that reached the library would fail differently (there is no GPU here)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    paths = torch.zeros((6, 8), dtype=torch.int32)
    lens = torch.ones(6, dtype=torch.int32)
    bad = [                                                      # every case meets its own check: the message says which
        (paths, lens, "in device memory"),                       # CPU tensors, otherwise right
        (paths.to(torch.int64), lens.to(torch.int64), "torch.int32"),
        (paths.to(torch.int64), lens, "torch.int32"),
        (paths, lens.to(torch.int64), "torch.int32"),
        (paths.to(torch.float32), lens, "torch.int32"),
        (paths[:, ::2], lens, "contiguous"),                     # not contiguous
        (paths.t().contiguous().t(), lens, "contiguous"),
        (paths, torch.ones(12, dtype=torch.int32)[::2], "contiguous"),
        (paths, lens[:5], r"\[n, stride\] and lens \[n\]"),        # mismatched n
        (paths[:5], lens, r"\[n, stride\] and lens \[n\]"),
        (paths[0], lens, r"\[n, stride\] and lens \[n\]"),         # paths without its second dimension
        (paths, lens[:, None], r"\[n, stride\] and lens \[n\]"),
        (paths, None, "go together"),                            # paths without lens
        (None, lens, "go together"),
        (paths.numpy(), lens.numpy(), "must be torch tensors"),  # not tensors at all
        (paths, lens.numpy(), "must be torch tensors"),
    ]
    for p, l, why in bad:
        with pytest.raises(TypeError, match=why):
            e.skipgram(3, 2, paths=p, lens=l)


def test_numpy_philox_is_the_oracles(oracle):
    rng = np.random.default_rng(5)
    F = 0xFFFFFFFF
    cases = [((0, 0, 0, 0), (0, 0)), ((F, F, F, F), (F, F)), ((F, F, F, F), (7, 1)), ((F, F, F, F), (F, 1)), ((0, 0, 0, 0), (F, 1)),
             ((1, 2, 3, 4), (5, 1)), ((F, 0, F, 0), (0, 1)), ((0, F, 0, F), (1, 1))]
    for _ in range(40):
        c = tuple(int(x) for x in rng.integers(0, 2**32, size=4))
        cases.append((c, (int(rng.integers(0, 2**32)), 1)))
        cases.append((c, tuple(int(x) for x in rng.integers(0, 2**32, size=2))))
    ctr = np.array([c for c, _ in cases], dtype=np.uint64)
    key = np.array([k for _, k in cases], dtype=np.uint64)
    got = np.stack(ref.philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    for i, (c, k) in enumerate(cases):
        assert [int(x) for x in got[i]] == oracle.philox(c, k), (c, k)


def test_the_index_map_at_the_ends_of_the_word_range():
    for n_v in (1, 2, 3, 34, 12520, 2**31 - 1):
        assert int(ref.index_of(0, n_v)) == 0
        assert int(ref.index_of(0xFFFFFFFF, n_v)) == n_v - 1
    assert int(ref.index_of(0x80000000, 1)) == 0 and int(ref.index_of(0x80000000, 34)) == 17
    words = np.arange(0, 2**32, 2**20 + 12345, dtype=np.uint64)
    idx = ref.index_of(words, 7)
    assert idx.min() == 0 and idx.max() == 6 and np.all(np.diff(idx.astype(np.int64)) >= 0)


def test_the_two_forms_of_the_window_restatement_agree():
    rng = np.random.default_rng(9)
    stride = 9
    lens = rng.integers(1, stride + 1, size=40).astype(np.int32)
    paths = np.full((40, stride), -1, dtype=np.int32)
    for r, l in enumerate(lens):
        paths[r, :l] = rng.integers(0, 1000, size=l)
    for C in (1, 2, 4, 9):
        a, b = ref.windows_loop(paths, lens, C), ref.windows_fast(paths, lens, C)
        assert a.shape == (int(ref.counts(lens, C).sum()), C) and np.array_equal(a, b) and (a >= 0).all()
        r, j = ref.window_keys(lens, C)
        assert np.array_equal(paths[r, j], a[:, 0])
