"""CPU: the host side of near-duplicate detection - clip.connected_components (union-find, minimum-index labels),
clip.group_split (whole groups, the size rule, the trainer's split on singletons), the exported names, and the fixed-radius
C entries refusing bad arguments before anything touches a device."""
import ctypes

import pytest
import torch



def test_connected_components_label_by_minimum():
    import clip
    pairs = torch.tensor([[5, 7], [2, 5], [8, 9], [1, 1], [7, 3]])
    assert clip.connected_components(10, pairs).tolist() == [0, 1, 2, 2, 4, 2, 6, 2, 8, 8]
    assert clip.connected_components(3, torch.empty(0, 2, dtype=torch.int64)).tolist() == [0, 1, 2]
    assert clip.connected_components(0, torch.empty(0, 2, dtype=torch.int64)).shape == (0,)
    # a chain met from the far end: every row still carries the minimum
    chain = torch.tensor([[n, n + 1] for n in range(98, -1, -1)])
    assert clip.connected_components(100, chain).tolist() == [0] * 100


def test_group_split_moves_whole_groups_until_the_target():
    import clip
    groups = torch.tensor([0, 0, 2, 3, 3, 3, 6, 7, 8, 9, 6, 11])
    for seed in range(20):
        train, val = clip.group_split(groups, 0.25, seed)                      # target: round(3.0) = 3 rows
        assert train == sorted(train) and val == sorted(val) and sorted(train + val) == list(range(12))
        assert not set(groups[train].tolist()) & set(groups[val].tolist())
        assert 3 <= len(val) <= 5 and train
        assert clip.group_split(groups, 0.25, seed) == (train, val)
    # the last group of the permutation never moves
    train, val = clip.group_split(torch.tensor([0, 0, 0, 3]), 0.9, 1)
    assert sorted(train + val) == [0, 1, 2, 3] and train and val
    with pytest.raises(ValueError, match="one group"):
        clip.group_split(torch.zeros(5, dtype=torch.int64), 0.5, 1)
    with pytest.raises(ValueError, match="positive"):
        clip.group_split(torch.arange(5), 0.0, 1)
    with pytest.raises(ValueError, match="label per row"):
        clip.group_split(torch.zeros(5, 2, dtype=torch.int64), 0.5, 1)


@pytest.mark.parametrize("N,frac,seed", [(64, 0.25, 567), (806, 0.1, 567), (7, 0.5, 2), (5, 0.99, 9), (3, 0.01, 4), (2, 0.5, 0)])
def test_group_split_of_singletons_is_the_trainers_split(N, frac, seed):
    """with every group of size 1: exactly what scripts/train_caption.py --val-fraction draws"""
    import clip
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed)).tolist()
    n_val = min(N - 1, max(1, int(round(frac * N))))
    train, val = clip.group_split(torch.arange(N), frac, seed)
    assert val == sorted(perm[:n_val]) and train == sorted(perm[n_val:])


def test_public_names():
    import clip
    from cclip_hip import ops
    assert callable(clip.group_split) and callable(clip.connected_components)
    for name in ("range_search", "duplicate_pairs", "duplicate_groups"):
        assert hasattr(clip.EmbeddingIndex, name)
    assert callable(ops.similarity_range) and callable(ops.similarity_range_workspace)


def test_workspace_rule_and_refusals_without_a_device():
    """arguments are checked before any launch: CCLIP_ERR_ARG (1) needs no GPU"""
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip import load_library
    lib = load_library()
    ws = lib.cclip_similarity_range_workspace
    ws.restype = ctypes.c_int64
    P, L, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float
    assert ws(I(4), L(100)) == 4 * 4                                           # one split
    assert ws(I(1), L(100003)) == 4 * 391                                      # ceil(100003 / 256) = 391 splits of 256 rows
    assert ws(I(60000), L(60000)) == 4 * 60000
    assert ws(I(0), L(5)) == 0 and ws(I(5), L(0)) == 0 and ws(I(5), L(2 ** 31)) == 0
    a = 1 << 20                                                                # an aligned address that is never dereferenced
    for fn in (lib.cclip_similarity_range_count, lib.cclip_similarity_range_count_f16):
        assert fn(P(a), L(64), I(4), P(a), L(64), L(4), I(40), F(0.5), I(0), P(a), L(1 << 20), P(0)) == 1
        assert fn(P(a), L(64), I(4), P(a + 4096), L(64), L(4), I(64), F(0.5), I(1), P(a), L(1 << 20), P(0)) == 1
        assert fn(P(a), L(64), I(4), P(a), L(64), L(4), I(64), F(0.5), I(0), P(a), L(8), P(0)) == 1
    for fn in (lib.cclip_similarity_range_emit, lib.cclip_similarity_range_emit_f16):
        assert fn(P(a), L(64), I(4), P(a), L(64), L(4), I(64), F(0.5), I(0), P(a), L(5), L(4), P(a), P(a), P(0)) == 1
        assert fn(P(a), L(64), I(4), P(a), L(64), L(4), I(64), F(0.5), I(0), P(a), L(0), L(4), P(0), P(a), P(0)) == 1
        assert fn(P(a), L(64), I(4), P(a), L(64), L(4), I(64), F(0.5), I(0), P(a), L(0), L(0), P(a), P(a), P(0)) == 0   # total 0: no launch
