"""clip.spread_labels end to end on the MI355X, on planted clusters (tests/label_spread_ref.py: planted): the kNN graph the
device finds goes through the float64 pipeline reference, whose propagated bound the kernels' distributions must meet and whose
labels they must reproduce on every row; then the public surface: bf16 and fp16 stores, EmbeddingIndex.spread_labels,
suspects, unreachable rows, the early stop, bitwise repeatability and one run of scripts/propagate_labels.py.

On the three planted configurations the float64 reference gives unlabelled accuracy 1.0 and a smallest top-two margin of 1.0
(the clusters are separate components of the kNN graph: tests/test_label_spread_cpu.py asserts both); the change of its 50th
step is 0.6e-5 to 2.5e-5, alpha^50 of the first, not the 1e-7 first hoped for, and nothing here depends on it.
test_overlapping_clusters adds a set whose clusters touch, so that mixed distributions meet the bound too."""
import functools
import json
import os
import sys

import pytest
import torch

import label_spread_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

CONFIGS = [(600, 6, 1.0, 3), (257, 2, 0.6, 2), (300, 9, 0.8, 1)]                  # N, classes, noise, labelled per class
K, BETA, ALPHA, ITERS = 10, 5.5, 0.9, 50


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@functools.lru_cache(maxsize=None)
def case(N, Cn, noise, per, dtype):
    """the planted rows, the device's kNN graph of them and the float64 pipeline from that graph (computed once, not changed)"""
    import clip
    rows, truth, labels = R.planted(N, Cn, noise, per, seed=100 + N, dtype=dtype)
    index = clip.EmbeddingIndex(rows.float(), dtype=dtype)
    scores, idx = index.knn_graph(K)
    ref = R.pipeline_ref(scores.cpu(), idx.cpu(), labels, max(2, Cn), BETA, ALPHA, ITERS)
    return index, truth, labels, ref


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("N,Cn,noise,per", CONFIGS)
def test_planted_clusters(N, Cn, noise, per, dtype):
    import clip
    index, truth, labels, ref = case(N, Cn, noise, per, dtype)
    fin = ref["finish"]
    assert fin["decided"].all() and not fin["zero"].any()                         # the reference leaves no row undecided
    un = labels < 0
    assert torch.equal(fin["pred"][un], truth[un])                                # and labels every unlabelled row rightly
    res = clip.spread_labels(index, labels, n_classes=max(2, Cn), k=K, beta=BETA, alpha=ALPHA, n_iter=ITERS)
    err = (res.distributions.cpu().double() - fin["dist"]).abs()
    r = (err / ref["dist_tol"].clamp(min=1e-300)).max().item()
    print(f"[label spread] planted N{N} C{Cn} {dtype}: distributions, largest err / tol {r:.3f} (largest tol {ref['dist_tol'].max().item():.2e})")
    assert r <= 1.0
    assert torch.equal(res.pred.cpu(), fin["pred"])
    assert torch.equal(res.labels.cpu(), torch.where(un, fin["pred"], labels))
    assert res.n_iter == ITERS and res.delta is None and res.suspects.numel() == 0 and res.unreachable.numel() == 0
    assert res.pred.dtype == torch.int64 and res.distributions.shape == (N, max(2, Cn)) and res.distributions.is_cuda
    conf = res.confidence.cpu().double()
    assert (conf - fin["dist"].max(dim=1).values).abs().max().item() <= ref["dist_tol"].max().item()
    cert = res.certainty.cpu()
    assert ((cert >= -1e-6) & (cert <= 1.0)).all()
    # the method of the index is the function; two fresh calls are bitwise equal
    again = index.spread_labels(labels, n_classes=max(2, Cn), k=K, beta=BETA, alpha=ALPHA, n_iter=ITERS)
    for a, b in ((res.distributions, again.distributions), (res.confidence, again.confidence), (res.certainty, again.certainty)):
        assert same_bits(a, b)
    assert torch.equal(res.pred, again.pred) and torch.equal(res.labels, again.labels)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_overlapping_clusters(dtype):
    """the recipe's clusters are separate components of the kNN graph and their distributions one-hot; at noise 2.0 the
    clusters touch, mass crosses between them and every entry of the distributions is tested by the bound"""
    import clip
    rows, truth, labels = R.planted(600, 6, 2.0, 3, seed=900, dtype=dtype)
    index = clip.EmbeddingIndex(rows.float(), dtype=dtype)
    scores, idx = index.knn_graph(K)
    ref = R.pipeline_ref(scores.cpu(), idx.cpu(), labels, 6, BETA, ALPHA, ITERS)
    fin = ref["finish"]
    res = index.spread_labels(labels, n_classes=6, k=K, beta=BETA, alpha=ALPHA, n_iter=ITERS)
    assert ((fin["dist"] > 1e-3) & (fin["dist"] < 0.999)).double().mean().item() > 0.5          # the distributions are mixed
    r = ((res.distributions.cpu().double() - fin["dist"]).abs() / ref["dist_tol"].clamp(min=1e-300)).max().item()
    left_out = 1.0 - fin["decided"].double().mean().item()
    print(f"[label spread] overlapping {dtype}: distributions, largest err / tol {r:.3f}; share of pred left out {left_out:.4f}")
    assert r <= 1.0 and left_out <= 0.01
    assert torch.equal(res.pred.cpu()[fin["decided"]], fin["pred"][fin["decided"]])
    cert_err = (res.certainty.cpu().double() - fin["cert"]).abs().max().item()
    assert cert_err <= 20 * ref["dist_tol"].max().item() + fin["cert_tol"].max().item()         # |dH / dp| <= |log p| + 1 < 20 for p > 1e-8


def test_mislabelled_row_is_a_suspect():
    import clip
    index, truth, labels, _ = case(600, 6, 1.0, 3, torch.bfloat16)
    labels = labels.clone()
    labels[40:340] = truth[40:340]                                                # more labels, so that one wrong one is outvoted
    wrong = 77
    labels[wrong] = (truth[wrong] + 1) % 6
    res = clip.spread_labels(index, labels, k=K, class_balance=False)
    assert res.suspects.tolist() == [wrong] and res.pred[wrong].item() == truth[wrong].item()
    assert res.labels[wrong].item() == labels[wrong].item()                       # `labels` keeps what was given


def test_component_without_a_label_is_unreachable():
    import clip
    index, truth, labels, _ = case(300, 9, 0.8, 1, torch.bfloat16)
    labels = labels.clone()
    labels[truth == 4] = -1                                                       # class 4 loses its one labelled row
    res = clip.spread_labels(index, labels, n_classes=9, k=K)
    pred = res.pred.cpu()
    # the planted clusters are separate components of the kNN graph here: the reference says so
    scores, idx = index.knn_graph(K)
    ref = R.pipeline_ref(scores.cpu(), idx.cpu(), labels, 9, BETA, ALPHA, ITERS)
    assert ref["finish"]["zero"].any() and torch.equal(pred, ref["finish"]["pred"])
    lost = ref["finish"]["zero"]
    assert (pred[lost] == -1).all() and torch.equal(res.unreachable.cpu(), torch.nonzero(lost).flatten())
    assert (res.confidence.cpu()[lost] == 0).all() and (res.certainty.cpu()[lost] == 0).all()
    assert (res.distributions.cpu()[lost] == 0).all() and (res.labels.cpu()[lost] == -1).all()
    assert torch.isfinite(res.distributions).all()


def test_check_every_stops_early():
    import clip
    index, truth, labels, _ = case(257, 2, 0.6, 2, torch.bfloat16)
    full = clip.spread_labels(index, labels, k=K, n_iter=400, check_every=10, tol=0.0)
    assert full.n_iter == 400 and full.delta is not None and full.delta >= 0.0
    res = clip.spread_labels(index, labels, k=K, n_iter=400, check_every=10, tol=1e-6)
    assert res.n_iter % 10 == 0 and 10 <= res.n_iter < 400 and 0.0 <= res.delta < 1e-6
    same = clip.spread_labels(index, labels, k=K, n_iter=res.n_iter)              # measuring changes nothing
    assert same_bits(res.distributions, same.distributions) and same.delta is None
    assert torch.equal(res.pred, full.pred)


def test_script_on_a_synthetic_pickle(tmp_path, capsys):
    import propagate_labels as M
    from clip_caption.data import save_embeddings
    rows, truth, labels = R.planted(300, 9, 0.8, 15, seed=400)
    import _common as C
    caps = [{"file_name": f"images/{i:04d}.png", "clip_embedding": i, "violation_type": C.CLASSES[int(truth[i])] if labels[i] >= 0 else ""}
            for i in range(300)]
    caps[20]["violation_type"] = C.CLASSES[(int(truth[20]) + 1) % 9]              # one of the 135 labelled rows is wrong
    pkl, out = str(tmp_path / "e.pkl"), str(tmp_path / "rows.json")
    save_embeddings(pkl, rows.float(), caps)
    lines, suspects, summary = M.main(["--index", pkl, "--label-key", "violation_type", "--k", "10", "--suspects", "--write-labels", out,
                                       "--min-confidence", "0.5", "--no-class-balance"])
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 300 - 135 and len(printed) == len(lines) + len(suspects) + 1
    assert set(lines[0]) == {"row", "file_name", "label", "confidence", "certainty"}
    names = sorted(C.CLASSES)
    right = sum(1 for ln in lines if ln["label"] == C.CLASSES[int(truth[ln["row"]])])
    assert right >= 0.95 * len(lines) and summary["classes"] == names and summary["labelled"] == 135
    assert [s["suspect"] for s in suspects] == [20] and suspects[0]["propagated"] == C.CLASSES[int(truth[20])]
    written = json.load(open(out))
    assert len(written) == 300 and written[0]["inherited"] is False and written[0]["label"] == caps[0]["violation_type"]
    assert written[200]["inherited"] is True and written[200]["label"] == C.CLASSES[int(truth[200])]
