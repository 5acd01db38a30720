"""srw_sgns_step and Engine.sgns_step / sgns_grad / train_sgns — what can be checked without a GPU: the symbol, its declaration, the
struct, the refusals that come before a handle or a device is touched, and the footing of the numpy restatement the GPU tests hold
every output element against (tests/sgns_ref.py): its gradients against torch.autograd in float64, and that the derived tolerance
notices a wrong update — a dropped negative, a flipped g — by a factor of at least 100 on the inputs tests/test_gpu_sgns.py uses."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import negatives_ref as nref
import sgns_ref as sref
import skipgram_ref as ref
from conftest import KARATE, ROOT
from helpers import pkg


def test_the_library_exports_the_entry_point():
    P = pkg()
    assert "srw_sgns_step" in P.EXPORTS and hasattr(P.lib(), "srw_sgns_step")


def test_the_header_declares_the_struct_and_the_function():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "stellar_rw.h")).read())
    assert ("typedef struct { int32_t context; int32_t num_negatives; int32_t dim; int32_t center; float lr; int32_t reserved; } "
            "srw_sgns_params;") in flat
    assert ("int32_t srw_sgns_step(srw_handle *h, const void *d_pos, const void *d_neg, int64_t n_windows, const srw_sgns_params *sp, "
            "const void *d_in, const void *d_out, void *d_in_new, void *d_out_new, int64_t n_rows, "
            "void *d_loss /* float32 [n_windows] or NULL */, int64_t *n_skipped /* or NULL */);") in flat
    assert "NO clamp" in flat and "NO sigmoid table" in flat and "word2vec.c" in flat       # the deliberate difference is stated


def test_the_kernel_is_on_the_build_list():
    csrc = os.path.join(ROOT, "stellar-random-walk_amd", "csrc")
    assert re.search(r"^HIP_SRC\s*:=.*\bsgns\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert os.path.exists(os.path.join(csrc, "sgns.hip"))


def test_the_struct_has_the_declared_fields_and_size():
    P = pkg()
    assert [f[0] for f in P.SgnsParams._fields_] == ["context", "num_negatives", "dim", "center", "lr", "reserved"]
    assert C.sizeof(P.SgnsParams) == 24
    sp = P.SgnsParams(5, 7, 128, 2, 0.025, 0)
    assert (sp.context, sp.num_negatives, sp.dim, sp.center, sp.reserved) == (5, 7, 128, 2, 0) and sp.lr == np.float32(0.025)
    assert P.SgnsParams.lr.offset == 16 and P.SgnsParams.reserved.offset == 20


def test_null_arguments_are_refused_not_touched():
    """No handle can exist here (srw_create needs a device): what is reachable is the refusal of a NULL h / sp."""
    P = pkg()
    L = P.lib()
    sp, n = P.SgnsParams(2, 0, 64, 0, 0.025, 0), C.c_int64(-7)
    assert L.srw_sgns_step(None, None, None, 0, C.byref(sp), None, None, None, None, 0, None, C.byref(n)) == P.ERR_INVALID
    assert L.srw_sgns_step(None, None, None, 0, None, None, None, None, None, 0, None, None) == P.ERR_INVALID
    assert n.value == -7


def test_engine_methods_have_the_agreed_parameters():
    E = pkg().Engine
    sig = inspect.signature(E.sgns_step)
    assert list(sig.parameters) == ["self", "pos", "neg", "emb_in", "emb_out", "lr", "center", "into", "loss"]
    assert [sig.parameters[k].default for k in ("center", "into", "loss")] == [0, None, False]
    sig = inspect.signature(E.sgns_grad)
    assert list(sig.parameters) == ["self", "pos", "neg", "emb_in", "emb_out", "center"] and sig.parameters["center"].default == 0
    sig = inspect.signature(E.train_sgns)
    assert list(sig.parameters) == ["self", "dim", "context", "num_negatives", "epochs", "batch_sources", "lr", "seed", "walk_kw"]
    assert (sig.parameters["lr"].default, sig.parameters["seed"].default) == (0.025, 1)
    assert sig.parameters["walk_kw"].kind is inspect.Parameter.VAR_KEYWORD


def test_tensor_arguments_are_refused_before_the_library_is_called():
    """An Engine without a handle: anything that reached the library would fail differently (there is no GPU here)."""
    P = pkg()
    e = P.Engine.__new__(P.Engine)
    e.h, e.device = None, 0
    pos = torch.zeros((6, 3), dtype=torch.int32)
    neg = torch.zeros((6, 2), dtype=torch.int32)
    tin = torch.zeros((4, 64), dtype=torch.float32)
    tout = torch.zeros((4, 64), dtype=torch.float32)
    bad = [
        (pos, neg, tin, tout, None, "in device memory"),
        (pos, None, tin, tout, None, "in device memory"),
        (pos.to(torch.int64), neg, tin, tout, None, r"pos must be torch\.int32"),
        (pos, neg.to(torch.int64), tin, tout, None, r"neg must be torch\.int32"),
        (pos, neg, tin.double(), tout, None, r"emb_in must be torch\.float32"),
        (pos, neg, tin, tout.half(), None, r"emb_out must be torch\.float32"),
        (pos[:, ::2], neg, tin, tout, None, "pos must be contiguous"),
        (pos, neg, tin[:, ::2], tout[:, ::2], None, "emb_in must be contiguous"),
        (pos[0], neg, tin, tout, None, r"\[W, C\] and neg \[W, K\]"),
        (pos, neg[:5], tin, tout, None, r"\[W, C\] and neg \[W, K\]"),
        (pos, neg[:, 0], tin, tout, None, r"\[W, C\] and neg \[W, K\]"),
        (pos, neg, tin, tout[:3], None, r"all be \[nV, D\]"),
        (pos, neg, tin[0], tout[0], None, r"all be \[nV, D\]"),
        (pos, neg, tin, tout, (tin,), "into must be a pair"),
        (pos, neg, tin, tout, tin, "into must be a pair"),
        (pos, neg, tin, tout, (tin.clone(), tout[:3].clone()), r"all be \[nV, D\]"),
        (pos, neg, tin, tout, (tin.clone(), tout.double()), r"into\[1\] must be torch\.float32"),
        (pos.numpy(), neg, tin, tout, None, "pos must be a torch tensor"),
        (pos, neg, tin.numpy(), tout, None, "emb_in must be a torch tensor"),
        (pos, neg, tin, tout, (tin.clone(), None), r"into\[1\] must be a torch tensor"),
    ]
    for p, n, a, b, into, why in bad:
        with pytest.raises(TypeError, match="sgns_step.*" + why):
            e.sgns_step(p, n, a, b, 0.025, into=into)
    with pytest.raises(TypeError, match="sgns_grad.*in device memory"):
        e.sgns_grad(pos, neg, tin, tout)
    with pytest.raises(TypeError, match=r"sgns_grad.*emb_in must be torch\.float32"):
        e.sgns_grad(pos, neg, tin.double(), tout)


# ---- the restatement's own footing --------------------------------------------------------------------------------------------------
def test_slots_and_skipped_windows():
    V = np.array([-5, 1, 2, 7, 9], dtype=np.int32)
    assert sref.slots_of(V, [[-5, 9], [0, 8], [-6, 10], [7, -1]]).tolist() == [[0, 4], [-1, -1], [-1, -1], [3, -1]]
    tin, tout = sref.tables(5, 64, 1)
    pos = np.array([[1, 2], [1, 3], [7, 9], [2, 2]], dtype=np.int32)      # 3 is in a gap
    neg = np.array([[9], [9], [-1], [-5]], dtype=np.int32)
    r = sref.step(V, pos, neg, tin, tout, 0.1, 0, tin, tout)
    assert r.skipped == 2 and r.ok.tolist() == [True, False, False, True] and r.loss[1] == 0 and r.loss[2] == 0 and r.loss[0] > 0
    only = sref.step(V, pos[[0, 3]], neg[[0, 3]], tin, tout, 0.1, 0, tin, tout)
    assert np.array_equal(only.new_in, r.new_in) and np.array_equal(only.new_out, r.new_out)
    assert r.m_in.tolist() == [0, 2, 2, 0, 0] and r.m_out.tolist() == [1, 0, 2, 0, 1]     # T = 2 terms per window on its centre


@pytest.mark.parametrize("one_table", [False, True])
def test_gradients_equal_autograd_in_float64(one_table):
    """zeroed new tables and lr = -1 give dLoss/d in and dLoss/d out of Loss = sum of -logsigmoid(+-f) over the same batch"""
    rng = np.random.default_rng(5)
    V = np.arange(10, 22, dtype=np.int32)
    C_, K, D, W = 4, 3, 64, 50
    pos = V[rng.integers(0, 12, size=(W, C_))]
    neg = V[rng.integers(0, 12, size=(W, K))]
    neg[0, 0] = pos[0, 1]                                    # a negative equal to its own centre (center = 1 below)
    tin, tout = sref.tables(12, D, 2, 0.5, 0.5)
    if one_table:
        tout = tin
    for center in (0, 1, 3):
        z = np.zeros((12, D))
        r = sref.step(V, pos, neg, tin, tout, -1.0, center, z, z if one_table else np.zeros((12, D)))
        a = torch.tensor(tin, dtype=torch.float64, requires_grad=True)
        b = a if one_table else torch.tensor(tout, dtype=torch.float64, requires_grad=True)
        sl = torch.as_tensor(sref.slots_of(V, np.concatenate([pos, neg], axis=1)))
        c = sl[:, center]
        t = torch.cat([sl[:, :center], sl[:, center + 1:]], dim=1)
        f = torch.einsum("wd,wtd->wt", a[c], b[t])
        sign = torch.tensor([1.0] * (C_ - 1) + [-1.0] * K, dtype=torch.float64)
        per_window = -torch.nn.functional.logsigmoid(sign * f).sum(dim=1)
        per_window.sum().backward()
        assert np.allclose(r.loss, per_window.detach().numpy(), rtol=1e-13, atol=0)
        assert np.allclose(r.new_in, a.grad.numpy(), rtol=1e-12, atol=1e-15)
        if not one_table:
            assert np.allclose(r.new_out, b.grad.numpy(), rtol=1e-12, atol=1e-15)


def test_softplus_and_sigmoid_stay_finite():
    x = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    assert np.isfinite(sref.softplus(x)).all() and np.isfinite(sref.sigmoid(x)).all()
    assert np.allclose(sref.softplus(x), [0.0, np.exp(-40.0), np.log(2.0), 40.0, 800.0], rtol=1e-15)
    assert sref.sigmoid(x).tolist() == [0.0, sref.sigmoid(np.array(-40.0)), 0.5, 1.0 / (1.0 + np.exp(-40.0)), 1.0]


def karate_batch(oracle, C_, K):
    """what Engine.skipgram_batch returns over KARATE_WALK on the device, from the CPU oracle's walk and the restatements of the
    windows and the draws (bit-identical: tests/test_gpu_parity.py, test_gpu_skipgram.py, test_gpu_negatives.py)"""
    g = oracle.Graph.load(KARATE, directed=False)
    paths, lens, _ = g.walk(**sref.KARATE_WALK)
    pos = ref.windows_fast(paths, lens, C_)
    neg = nref.negatives(lens, C_, K, sref.KARATE_SG["seed"], sref.KARATE_SG["epoch"], g.vertices())[0] if K else None
    return g.vertices(), pos[:sref.KARATE_W], None if neg is None else neg[:sref.KARATE_W]


def mutation_ratios(V, pos, neg, tin, tout, center, mutate, lr=sref.LR):
    """how far a wrong restatement lies outside the tolerance of the right one: the worst element of both tables and of loss"""
    want = sref.step(V, pos, neg, tin, tout, lr, center, tin, tout)
    got = sref.step(V, pos, neg, tin, tout, lr, center, tin, tout, mutate=mutate)
    return max(sref.worst(got.new_in, want.new_in, sref.table_bound(want, "in", tin)),
               sref.worst(got.new_out, want.new_out, sref.table_bound(want, "out", tout)),
               sref.worst(got.loss, want.loss, sref.loss_bound(want)))


@pytest.mark.parametrize("C_,K", sref.KARATE_SHAPES)
def test_the_tolerance_notices_a_wrong_update_on_the_karate_inputs(oracle, C_, K):
    V, pos, neg = karate_batch(oracle, C_, K)
    assert pos.shape == (sref.KARATE_W, C_)
    for D in (64, 512):
        tin, tout = sref.tables_for(V.size, D, 7)
        for center in sref.centers(C_):
            r = mutation_ratios(V, pos, neg, tin, tout, center, "flip_g")
            assert r >= 100, (D, center, r)
            if K:
                r = mutation_ratios(V, pos, neg, tin, tout, center, "drop_negative")
                assert r >= 100, (D, center, r)


def test_the_tolerance_notices_a_wrong_update_on_the_heavy_inputs():
    V, pos, neg = sref.heavy_windows()
    tin, tout = sref.tables(sref.HEAVY_NV, 64, 3, 0.5, 0.5)
    want = sref.step(V, pos, neg, tin, tout, sref.LR, 0, tin, tout)
    assert want.skipped == 0 and want.m_out.max() > 2000 and want.m_out.min() == 1 and want.m_in.max() > 2000
    for mutate in ("flip_g", "drop_negative"):
        assert mutation_ratios(V, pos, neg, tin, tout, 0, mutate) >= 100, mutate


def test_a_float32_evaluation_in_shuffled_order_stays_inside_the_tolerance():
    """the other side of the footing: float32 arithmetic as a kernel may order it does not trip the tolerance"""
    V, pos, neg = sref.heavy_windows()
    pos, neg = pos[:512], neg[:512]
    tin, tout = sref.tables(sref.HEAVY_NV, 64, 3, 0.5, 0.5)
    want = sref.step(V, pos, neg, tin, tout, sref.LR, 0, tin, tout)
    rng = np.random.default_rng(1)
    f32 = np.float32
    sl = sref.slots_of(V, np.concatenate([pos, neg], axis=1))
    new_in, new_out = tin.copy(), tout.copy()
    loss = np.zeros(len(pos), dtype=f32)
    for w in rng.permutation(len(pos)):
        c, t = sl[w, 0], sl[w, 1:]
        acc = np.zeros(64, dtype=f32)
        for i in rng.permutation(len(t)):
            perm = rng.permutation(64)
            f = f32(0)
            for d in perm:
                f = f32(f + f32(tin[c, d] * tout[t[i], d]))
            label = i < pos.shape[1] - 1
            x = -f if label else f
            s = f32(sref.sigmoid(np.float64(x)))
            g = f32(f32(sref.LR) * (s if label else -s))
            loss[w] = f32(loss[w] + f32(sref.softplus(np.float64(x))))
            acc = (acc + g * tout[t[i]]).astype(f32)
            new_out[t[i]] = (new_out[t[i]] + g * tin[c]).astype(f32)
        new_in[c] = (new_in[c] + acc).astype(f32)
    assert sref.worst(new_in, want.new_in, sref.table_bound(want, "in", tin)) < 1
    assert sref.worst(new_out, want.new_out, sref.table_bound(want, "out", tout)) < 1
    assert sref.worst(loss, want.loss, sref.loss_bound(want)) < 1
