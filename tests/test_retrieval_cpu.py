"""CPU: the hit rule of clip.retrieval_recall on hand-written index tensors (label matching, ks handling), and its argument
errors that are decided before anything touches the device."""
import pytest
import torch


def test_hit_rule_on_hand_written_indices():
    from clip.retrieval import recall_from_indices
    gallery_labels = torch.tensor([7, 7, 3, 5, 9, 3])
    query_labels = torch.tensor([3, 7, 9, 4])
    indices = torch.tensor([[0, 1, 2, 3],      # label 3 first met at rank 3
                            [1, 4, 0, 2],      # label 7 at rank 1
                            [0, 1, 2, 3],      # label 9 (row 4) never met
                            [5, 4, 3, 2]])     # label 4 is not in the gallery
    r = recall_from_indices(indices, query_labels, gallery_labels, (1, 2, 3, 4))
    assert r.dtype == torch.float64 and r.tolist() == [0.25, 0.25, 0.5, 0.5]
    # ks in any order, repeated, and a single k
    assert recall_from_indices(indices, query_labels, gallery_labels, (4, 1, 4)).tolist() == [0.5, 0.25, 0.5]
    assert recall_from_indices(indices, query_labels, gallery_labels, [3]).tolist() == [0.5]


def test_hit_rule_counts_a_query_once():
    from clip.retrieval import recall_from_indices
    gallery_labels = torch.tensor([1, 1, 1, 2])
    indices = torch.tensor([[0, 1, 2], [0, 1, 3]])
    r = recall_from_indices(indices, torch.tensor([1, 2]), gallery_labels, (1, 3))
    assert r.tolist() == [0.5, 1.0]


def test_pair_labels_are_arange():
    from clip.retrieval import recall_from_indices
    indices = torch.tensor([[0, 2], [2, 1], [0, 1]])
    lab = torch.arange(3)
    assert recall_from_indices(indices, lab, lab, (1, 2)).tolist() == [1 / 3, 2 / 3]


def test_hit_rule_argument_errors():
    from clip.retrieval import recall_from_indices
    indices = torch.zeros(2, 3, dtype=torch.int64)
    lab = torch.arange(2)
    for ks in ((), (0,), (4,), (1, 5)):
        with pytest.raises(ValueError, match="ks"):
            recall_from_indices(indices, lab, torch.arange(5), ks)
    with pytest.raises(ValueError, match="query_labels"):
        recall_from_indices(indices, torch.arange(3), torch.arange(5), (1,))


def test_recall_needs_labels_when_sizes_differ():
    import clip
    q, g = torch.randn(3, 64), torch.randn(5, 64)
    with pytest.raises(ValueError, match="Q = 3 and N = 5"):
        clip.retrieval_recall(q, g)
    with pytest.raises(ValueError, match="both"):
        clip.retrieval_recall(q, g, query_labels=torch.arange(3))
    with pytest.raises(ValueError, match="ks"):
        clip.retrieval_recall(q, g, ks=(1, 6), query_labels=torch.arange(3), gallery_labels=torch.arange(5))
    with pytest.raises(ValueError, match="ks"):
        clip.retrieval_recall(torch.randn(100, 64), torch.randn(100, 64), ks=(65,))


def test_public_names():
    import clip
    assert callable(clip.EmbeddingIndex) and callable(clip.retrieval_recall)
    for name in ("search", "search_text", "search_image", "add", "from_pickle"):
        assert hasattr(clip.EmbeddingIndex, name)
