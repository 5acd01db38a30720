"""srw_negative_weights_set / srw_graph_degrees_device / srw_path_vertex_counts / srw_skipgram_batch and their Engine methods — what can
be checked without a GPU: the symbols and their declarations, the struct, the refusals that come before a handle (or a device) is
touched, the Python signatures, and the numpy restatement's own footing (tests/negatives_ref.py).  The draws themselves:
tests/test_gpu_negatives.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import negatives_ref as nref
from conftest import ROOT
from helpers import pkg

NEW = ["srw_negative_weights_set", "srw_graph_degrees_device", "srw_path_vertex_counts", "srw_skipgram_batch"]


def test_the_library_exports_the_entry_points():
    P = pkg()
    L = P.lib()
    for s in NEW:
        assert s in P.EXPORTS and hasattr(L, s), s


def test_the_header_declares_the_struct_and_the_functions():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "stellar_rw.h")).read())
    assert ("typedef struct { int32_t context; int32_t num_negatives; uint32_t seed; uint32_t epoch; int32_t exclude_window; "
            "int32_t max_draws; } srw_skipgram_batch_params;") in flat
    assert "int32_t srw_negative_weights_set(srw_handle *h, const void *d_w, int64_t n);" in flat
    assert "int32_t srw_graph_degrees_device(srw_handle *h, void *d_out);" in flat
    assert ("int32_t srw_path_vertex_counts(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride, "
            "void *d_counts, int64_t *n_unknown);") in flat
    assert ("int32_t srw_skipgram_batch(srw_handle *h, const void *d_paths, const void *d_lens, int64_t n, int64_t stride, "
            "const srw_skipgram_batch_params *bp, void *d_pos, void *d_neg, int64_t cap_windows, int64_t *n_windows);") in flat
    assert "the last attempt's vertex stands" in flat          # the documented end of the redraw loop
    assert "not filtered" in flat.lower()                      # ... and srw_skipgram_windows' sentence stays: it is still true of that entry


def test_the_kernels_are_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bnegatives\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    src = open(os.path.join(csrc, "negatives.hip")).read()
    for k in ("k_neg_draw", "k_neg_guide", "k_vertex_count", "rocprim::inclusive_scan", "__umul64hi"):
        assert k in src, k
    assert "skipgram_batch(" in open(os.path.join(csrc, "engine.h")).read()


def test_the_struct_has_the_declared_fields_and_size():
    P = pkg()
    assert [f[0] for f in P.SkipgramBatchParams._fields_] == ["context", "num_negatives", "seed", "epoch", "exclude_window", "max_draws"]
    assert C.sizeof(P.SkipgramBatchParams) == 24
    bp = P.SkipgramBatchParams(3, 2, 0xFFFFFFFF, 7, 1, 16)
    assert (bp.context, bp.num_negatives, bp.seed, bp.epoch, bp.exclude_window, bp.max_draws) == (3, 2, 0xFFFFFFFF, 7, 1, 16)
    assert P.SkipgramBatchParams.max_draws.offset == 20 and P.SkipgramBatchParams.exclude_window.offset == 16


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of NULL h / bp / n_windows / n_unknown,
    which comes before the handle is looked at."""
    P = pkg()
    L = P.lib()
    bp, w = P.SkipgramBatchParams(2, 0, 1, 0, 0, 8), C.c_int64(-7)
    assert L.srw_skipgram_batch(None, None, None, 0, 0, C.byref(bp), None, None, 0, C.byref(w)) == P.ERR_INVALID
    assert L.srw_skipgram_batch(None, None, None, 0, 0, None, None, None, 0, None) == P.ERR_INVALID
    assert L.srw_negative_weights_set(None, None, 0) == P.ERR_INVALID
    assert L.srw_graph_degrees_device(None, None) == P.ERR_INVALID
    assert L.srw_path_vertex_counts(None, None, None, 0, 0, None, C.byref(w)) == P.ERR_INVALID
    assert L.srw_path_vertex_counts(None, None, None, 0, 0, None, None) == P.ERR_INVALID
    assert w.value == -7


def test_engine_methods_have_the_agreed_parameters():
    P = pkg()
    E = P.Engine
    assert list(inspect.signature(E.degrees_tensor).parameters) == ["self"]
    sig = inspect.signature(E.visit_counts)
    assert list(sig.parameters) == ["self", "paths", "lens"] and [p.default for p in list(sig.parameters.values())[1:]] == [None, None]
    assert list(inspect.signature(E.set_negative_weights).parameters) == ["self", "weights"]
    sig = inspect.signature(E.skipgram_batch)
    assert list(sig.parameters) == ["self", "context", "num_negatives", "seed", "epoch", "paths", "lens", "exclude_window", "max_draws"]
    assert [sig.parameters[k].default for k in ("num_negatives", "seed", "epoch", "paths", "lens", "exclude_window", "max_draws")] == \
        [0, 1, 0, None, None, False, 8]
    sig = inspect.signature(E.walk_skipgram_batch)
    assert list(sig.parameters)[:3] == ["self", "sources", "context"] and list(sig.parameters)[-1] == "walk_kw"
    assert sig.parameters["walk_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert sig.parameters["exclude_window"].default is False and sig.parameters["max_draws"].default == 8
    # the existing methods keep theirs
    assert list(inspect.signature(E.skipgram).parameters) == ["self", "context", "num_negatives", "seed", "epoch", "paths", "lens"]
    assert "pow(0.75)" in E.set_negative_weights.__doc__          # the recipes


def test_tensor_arguments_are_refused_before_the_library_is_called():
    """An Engine without a handle: anything that reached the library would fail differently (there is no GPU here)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    paths = torch.zeros((6, 8), dtype=torch.int32)
    lens = torch.ones(6, dtype=torch.int32)
    bad = [
        (paths, lens, "in device memory"),
        (paths.to(torch.int64), lens, "torch.int32"),
        (paths, lens.to(torch.int64), "torch.int32"),
        (paths[:, ::2], lens, "contiguous"),
        (paths, lens[:5], r"\[n, stride\] and lens \[n\]"),
        (paths[0], lens, r"\[n, stride\] and lens \[n\]"),
        (paths, None, "go together"),
        (None, lens, "go together"),
        (paths.numpy(), lens.numpy(), "must be torch tensors"),
    ]
    for p, l, why in bad:
        with pytest.raises(TypeError, match="skipgram_batch.*" + why):
            e.skipgram_batch(3, 2, paths=p, lens=l, exclude_window=True)
        with pytest.raises(TypeError, match="visit_counts.*" + why):
            e.visit_counts(paths=p, lens=l)
    wbad = [
        (np.ones(4), TypeError, "torch tensor"),
        ([1, 2, 3], TypeError, "torch tensor"),
        (torch.ones((2, 2)), TypeError, "one-dimensional"),
        (torch.ones(3, dtype=torch.bool), TypeError, "integer or floating"),
        (torch.ones(3), TypeError, "in device memory"),              # a CPU tensor, otherwise right
        (torch.ones(3, dtype=torch.int64), TypeError, "in device memory"),
        (torch.tensor([1.0, -0.5]), ValueError, "negative or not finite"),
        (torch.tensor([1.0, float("nan")]), ValueError, "negative or not finite"),
        (torch.tensor([1.0, float("inf")]), ValueError, "negative or not finite"),
        (torch.tensor([1, -1]), ValueError, "below 0"),
        (torch.tensor([1, 2**32]), ValueError, r"at or above 2\^32"),
    ]
    for w, exc, why in wbad:
        with pytest.raises(exc, match=why):
            e.set_negative_weights(w)


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
TABLES = [
    [0, 0, 3, 0, 0, 5, 1, 0, 0],            # leading, interior and trailing zeros
    [7],
    [0, 0, 1],
    [1, 0, 0],
    [2**32 - 1, 0, 2**32 - 1, 1],
    [1, 1, 1, 1, 1],
]


def test_searchsorted_selects_what_a_linear_scan_selects():
    for w in TABLES:
        cdf = nref.cdf_of(w)
        T = int(cdf[-1])
        assert cdf.dtype == np.uint64 and T == sum(w)
        ts = sorted(set([0, T - 1] + [int(c) for c in cdf if int(c) < T] + [max(int(c) - 1, 0) for c in cdf]))
        for t in ts:
            i = int(nref.select(cdf, t))
            assert i == nref.select_linear(cdf, t) and w[i] > 0, (w, t)
        assert np.array_equal(nref.select(cdf, np.array(ts, dtype=np.uint64)), [nref.select_linear(cdf, t) for t in ts])


def test_the_ends_of_the_draw_range():
    """t = 0 gives the first positive-weight index, u = 2^64 - 1 the last"""
    for w in TABLES:
        cdf = nref.cdf_of(w)
        T = int(cdf[-1])
        pos = [i for i, x in enumerate(w) if x > 0]
        assert int(nref.select(cdf, 0)) == pos[0]
        t_max = nref.hi64_int(2**64 - 1, T)
        assert t_max == T - 1 and int(nref.select(cdf, t_max)) == pos[-1]
        assert nref.hi64_int(0, T) == 0


def test_the_two_forms_of_the_high_product_agree():
    rng = np.random.default_rng(17)
    for T in [1, 2, 3, 34, 2**32 - 1, 2**32, 2**32 + 1, 2**48 + 12345, 90127 * (2**32 - 1), 2**59 - 1, 2**59]:
        hi = rng.integers(0, 2**32, size=200, dtype=np.uint64)
        lo = rng.integers(0, 2**32, size=200, dtype=np.uint64)
        hi[:4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
        lo[:4] = [0, 0xFFFFFFFF, 0, 0xFFFFFFFF]
        got = nref.hi64_split(hi, lo, T)
        want = [nref.hi64_int((int(a) << 32) | int(b), T) for a, b in zip(hi, lo)]
        assert [int(x) for x in got] == want, T
        assert max(want) < T


def test_the_restatement_redraws_and_counts():
    """a two-vertex table whose window holds both: every attempt is rejected, the last one stands"""
    lens = np.array([3, 2], dtype=np.int32)
    paths = np.array([[5, 9, 5], [9, 5, -1]], dtype=np.int32)
    V = np.array([5, 9], dtype=np.int32)
    for w in (None, [1, 3]):
        plain, rd0, ex0 = nref.negatives(lens, 2, 3, 4, 1, V, w=w)
        assert plain.shape == (3, 3) and (rd0, ex0) == (0, 0)
        for md in (1, 2, 16):
            neg, rd, ex = nref.negatives(lens, 2, 3, 4, 1, V, w=w, paths=paths, exclude=True, max_draws=md)
            assert (rd, ex) == (9 * (md - 1), 9)
            cdf = None if w is None else nref.cdf_of(w)
            r, j = np.array([0, 0, 1]), np.array([0, 1, 0])
            for k in range(3):
                assert np.array_equal(neg[:, k], nref.draw(r, j, k, md - 1, 4, 1, V, cdf))
        assert np.array_equal(nref.negatives(lens, 2, 3, 4, 1, V, w=w, paths=paths, exclude=True, max_draws=1)[0], plain)
    # a weight of zero is never drawn
    neg, _, _ = nref.negatives(np.full(50, 6, dtype=np.int32), 2, 5, 1, 0, np.array([1, 2, 3, 4], dtype=np.int32), w=[0, 2, 0, 1])
    assert set(np.unique(neg).tolist()) == {2, 4}
