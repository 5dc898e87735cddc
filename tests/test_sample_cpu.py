"""CPU: the float64 helper of the row-sampling tests (tests/sample_ref.py) against the reference's nucleus filter written out
literally (CLIP_prefix_caption/test.py:492-500), and the argument checks of ops.sample_rows that run before the library is
touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sample_ref import draw_ref, sample_rows_ref  # noqa: E402


def _rows(seed, n, V, ties):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, V, generator=g) * 3
    if ties:
        x = (x * 2).round() / 2
    return x


def _literal_filter(row64, top_p):
    """test.py:492-500 on one row of float64 logits (already temperature-scaled): the ids that survive"""
    logits = torch.from_numpy(row64)
    sorted_logits, sorted_indices = torch.sort(logits, descending=True, stable=True)     # (stable: equal logits by ascending id)
    cumulative_probs = torch.cumsum(torch.softmax(sorted_logits, dim=-1), dim=-1)
    sorted_indices_to_remove = cumulative_probs > top_p
    sorted_indices_to_remove[..., 1:] = sorted_indices_to_remove[..., :-1].clone()
    sorted_indices_to_remove[..., 0] = 0
    return set(sorted_indices[~sorted_indices_to_remove].tolist())


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("inv_t", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("top_p", [0.3, 0.8, 0.95])
def test_kept_set_is_the_reference_filter(ties, inv_t, top_p):
    x = _rows(11, 6, 257, ties)
    for row, ref in zip(x.numpy(), sample_rows_ref(x.numpy(), inv_t, 0, top_p)):
        want = _literal_filter(row.astype(np.float64) * inv_t, top_p)
        assert set(ref.kept().tolist()) == want
        assert ref.n_kept() == len(want)
        assert abs(ref.p.sum() - 1) < 1e-12 and ref.ahead[0] == 0.0


def test_order_breaks_ties_by_id_and_top_k_cuts_it():
    x = np.array([[1.0, 3.0, 3.0, -0.0, 0.0, 3.0, float("-inf")]], dtype=np.float32)
    ref = sample_rows_ref(x, 1.0, 2, 1.0)[0]
    assert ref.order.tolist() == [1, 2, 5, 0, 3, 4, 6]
    assert ref.kept().tolist() == [1, 2] and ref.p[6] == 0.0
    assert sample_rows_ref(x, 1.0, 0, 1.0)[0].n_kept() == 7 and sample_rows_ref(x, 1.0, 99, 1.0)[0].n_kept() == 7


@pytest.mark.parametrize("ties", [False, True])
def test_top_k_1_and_tiny_top_p_keep_only_the_argmax(ties):
    x = _rows(12, 8, 300, ties)
    first_max = x.argmax(dim=1)                                          # torch: the first maximum = the lowest id
    for kw in (dict(top_k=1, top_p=1.0), dict(top_k=0, top_p=1e-6)):
        for i, ref in enumerate(sample_rows_ref(x.numpy(), 1.0, **kw)):
            assert ref.kept().tolist() == [int(first_max[i])]
            for u in (0.0, 0.5, 1 - 2.0 ** -24):
                assert draw_ref(ref, u)[0] == int(first_max[i])


def test_draw_walks_ids_in_ascending_order():
    x = np.log(np.array([[0.1, 0.4, 0.2, 0.3]], dtype=np.float64)).astype(np.float32)
    ref = sample_rows_ref(x, 1.0, 0, 1.0)[0]
    assert [draw_ref(ref, u)[0] for u in (0.0, 0.09, 0.11, 0.49, 0.51, 0.69, 0.71, 0.999)] == [0, 0, 1, 1, 2, 2, 3, 3]
    ref = sample_rows_ref(x, 1.0, 2, 1.0)[0]                             # kept {1, 3}: masses 4/7 and 3/7 of Z = 0.7
    assert [draw_ref(ref, u)[0] for u in (0.0, 0.57, 0.58, 0.99)] == [1, 1, 3, 3]
    assert abs(draw_ref(ref, 0.0)[1] - 0.7) < 1e-7


def test_ops_sample_rows_validates_before_the_library(monkeypatch):
    import cclip_hip._lib as L
    from cclip_hip import ops

    def boom():
        raise AssertionError("the library must not be touched")
    monkeypatch.setattr(L, "load_library", boom)
    logits, u, done = torch.zeros(2, 8), torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    for kw in (dict(inv_temperature=0.0), dict(inv_temperature=-1.0), dict(inv_temperature=float("inf")), dict(top_k=-1),
               dict(top_k=1.5), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ops.sample_rows(logits, u, done, **kw)
    for bad in ((logits.double(), u, done), (logits, u.double(), done), (logits, u, done.long()), (logits[0], u, done),
                (logits.t(), u, done), (logits, u[:1], done), (logits, u, done[:1]), (torch.zeros(0, 8), u[:0], done[:0]),
                (torch.zeros(1, 65537), u[:1], done[:1]), (logits, torch.zeros(4)[::2], done)):
        with pytest.raises(ValueError):
            ops.sample_rows(*bad)
    with pytest.raises(TypeError, match="cuda"):
        ops.sample_rows(logits, u, done)                                 # well-formed CPU tensors: there is no host path
    with pytest.raises(TypeError, match="cuda"):
        ops.sample_rows(logits, u, done, token=torch.zeros(2, dtype=torch.int32))


def test_frequency_seed_passes_its_bound_in_float64():
    """the seed of the GPU frequency test (tests/test_sample_rows_gpu.py) on the float64 helper and the same uniforms"""
    from sample_ref import FREQ_ROWS, frequency_bound_ok, frequency_case
    logits, u, p = frequency_case()
    ref = sample_rows_ref(logits[None], 1.0, 0, 1.0)[0]
    c = np.cumsum(ref.p)                                                 # all 64 kept, ids ascending, Z = 1
    tokens = np.minimum(np.searchsorted(c, u.astype(np.float64) * c[-1], side="right"), 63)
    assert tokens[0] == draw_ref(ref, float(u[0]))[0]
    ok, worst = frequency_bound_ok(np.bincount(tokens, minlength=64), p, FREQ_ROWS)
    print(f"largest deviation {worst:.2f} sigma")
    assert ok and worst < 4.0, worst                                     # (a sigma to spare for the kernel's fp32 cut points)


def test_generate_sample_argument_errors_need_no_device():
    from clip_caption import generate_sample, generate_sample_batch
    emb = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="num_samples"):
        generate_sample(None, None, embed=emb, num_samples=0)
    with pytest.raises(ValueError, match="entry_length"):
        generate_sample_batch(None, None, emb, entry_length=0)
    with pytest.raises(TypeError, match="cuda"):
        generate_sample(None, None, embed=emb)
    with pytest.raises(ValueError):
        generate_sample(None, None)
