"""clip.kmeans on the MI355X: the Lloyd loop against the float64 loop of tests/kmeans_ref.py on planted clusters, iteration by
iteration; seeding, n_init, reseed_empty, EmbeddingIndex.kmeans / assign, representatives, repeatability; and
scripts/cluster_images.py end to end.

Labels can only be compared where they are decided: the float64 loop is checked first, on the CPU - at every iteration every
row's margin (best minus second float64 score) must exceed 2 tol (tol = kmeans_ref.assign_tol, the derived bound of the
assignment kernel) and no cluster may be empty - and only then does the device run.
"""
import functools
import json
import os
import sys

import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = [torch.bfloat16, torch.float16]
SIZES = [40, 400, 90, 150, 60, 220, 75, 300]


@functools.lru_cache(maxsize=None)
def planted_case(D, dtype):
    """8 planted groups of 40 - 400 rows; the init: every direction mixed with its neighbour's, so that the loop needs three or
    four assignment steps (the mix per D is chosen so that no float64 margin on the way comes near 2 tol: the test asserts it)"""
    feats, truth, dirs = R.planted(SIZES, D, 0.6, 31 + D)
    init = dirs + {64: 1.2, 128: 0.8}[D] * dirs.roll(1, 0)
    return feats, truth, init / init.norm(dim=1, keepdim=True)


def same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        a, b = (a.view(torch.int16), b.view(torch.int16)) if a.element_size() == 2 else (a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


def results_equal(r1, r2):
    return all(same_bits(getattr(r1, f), getattr(r2, f)) for f in ("centroids", "labels", "scores", "margin", "counts", "concentration")) \
        and (r1.objective, r1.n_iter, r1.converged) == (r2.objective, r2.n_iter, r2.converged)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_lloyd_matches_the_float64_loop_on_planted_clusters(D, dtype):
    import clip
    from clip.retrieval import normalize_rows
    feats, truth, init = planted_case(D, dtype)
    x16 = normalize_rows(feats, dtype).cpu()                       # the rows the device clusters (normalised by its own kernel)
    c16 = normalize_rows(init, dtype).cpu()
    ref = R.lloyd_ref(x16, c16)
    for it, h in enumerate(ref["history"], start=1):               # the conditions, on the reference alone
        tol = R.assign_tol(D, x16, h["centroids"])
        margin = (h["best"] - h["second"]).min().item()
        print(f"[kmeans] D{D} {dtype} iteration {it}: min margin {margin:.3e}, 2 tol {2 * tol:.3e}, smallest cluster {int(h['counts'].min())}")
        assert margin > 2 * tol, f"iteration {it}: a row's margin is within 2 tol"
        assert (h["counts"] > 0).all(), f"iteration {it}: an empty cluster"
    assert ref["converged"] and ref["n_iter"] >= 3 and R.same_partition(ref["labels"], truth)
    for it, h in enumerate(ref["history"], start=1):
        got = clip.kmeans(feats, len(SIZES), init=init, max_iter=it, dtype=dtype)
        assert torch.equal(got.labels.cpu(), h["assign"]), f"iteration {it}: labels differ from the float64 loop"
        assert torch.equal(got.counts.cpu(), h["counts"]) and got.n_iter == it
    assert got.converged and R.same_partition(got.labels.cpu(), truth) and sorted(got.counts.tolist()) == sorted(SIZES)
    full = clip.kmeans(feats, len(SIZES), init=init, dtype=dtype)
    assert full.n_iter == ref["n_iter"] and full.converged and results_equal(full, got)
    tol = R.assign_tol(D, x16, full.centroids.cpu())
    assert (full.scores.cpu().double() - R.scores64(x16, full.centroids.cpu())[torch.arange(x16.shape[0]), full.labels.cpu()]).abs().max() <= tol
    assert abs(full.objective - ref["objective"]) <= 2.0 ** -7      # centroids one 16-bit step apart move a score by <= 2^-8
    assert (full.concentration.cpu().double() - ref["concentration"]).abs().max() <= 1e-3
    assert full.centroids.dtype == dtype and full.labels.dtype == torch.int64 and full.margin.dtype == torch.float32
    assert (full.margin > 0).all() and full.counts.dtype == torch.int64


def test_kmeans_plusplus_seeding():
    import clip
    from clip.cluster import _seed_plusplus
    feats, truth, _ = planted_case(64, torch.bfloat16)
    index = clip.EmbeddingIndex(feats)
    p1, p2, p3 = (_seed_plusplus(index.features, 8, s) for s in (0, 0, 1))
    assert p1.dtype == torch.int64 and p1.shape == (8,) and p1.unique().numel() == 8
    assert torch.equal(p1, p2) and not torch.equal(p1, p3)
    dup = torch.cat([feats[:3]] * 5)                                # 15 rows, 3 distinct: all weights reach 0, the draw stays legal
    picks = _seed_plusplus(clip.EmbeddingIndex(dup).features, 6, 0)
    assert picks.unique().numel() == 6
    a, b, c = (clip.kmeans(feats, 8, seed=s) for s in (0, 0, 1))
    assert results_equal(a, b), "the same seed gave another result"
    assert a.converged and c.converged
    print(f"[kmeans] kmeans++ seeds 0 / 1: objective {a.objective:.5f} / {c.objective:.5f}, iterations {a.n_iter} / {c.n_iter}")


def test_n_init_keeps_the_best_run():
    import clip
    feats, _, _ = planted_case(64, torch.bfloat16)
    singles = [clip.kmeans(feats, 8, init="random", seed=s) for s in (5, 6, 7)]
    best = clip.kmeans(feats, 8, init="random", seed=5, n_init=3)
    print(f"[kmeans] n_init: single objectives {[round(s.objective, 5) for s in singles]}, n_init=3 {best.objective:.5f}")
    assert all(best.objective >= s.objective for s in singles)
    from clip.cluster import pick_best_run
    assert results_equal(best, singles[pick_best_run([s.objective for s in singles])])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_reseed_empty(dtype):
    import clip
    from test_kmeans_cpu import reseed_case
    x16, truth, init = reseed_case(dtype)
    kept = clip.kmeans(x16.float(), 3, init=init.float(), reseed_empty=False, dtype=dtype)
    assert kept.counts.tolist() == [180, 0, 0] and kept.concentration[1:].tolist() == [0.0, 0.0] and kept.converged
    reseeded = clip.kmeans(x16.float(), 3, init=init.float(), reseed_empty=True, dtype=dtype)
    assert (reseeded.counts > 0).all() and reseeded.converged and reseeded.objective > kept.objective
    assert reseeded.counts.sum().item() == 180


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_index_kmeans_assign_and_representatives(dtype):
    import clip
    feats, truth, init = planted_case(128, dtype)
    index = clip.EmbeddingIndex(feats[:1000], dtype=dtype)
    a = index.kmeans(8, init=init)
    b = clip.kmeans(index.features, 8, init=init)
    c = index.kmeans(8, init=init)
    assert results_equal(a, b), "EmbeddingIndex.kmeans differs from kmeans(index.features)"
    assert results_equal(a, c), "two fresh calls differ"
    labels, scores = index.assign(a.centroids)                      # the stored rows: the result's own labels and scores
    assert labels.dtype == torch.int64 and torch.equal(labels, a.labels) and same_bits(scores, a.scores)
    held = clip.EmbeddingIndex(feats[1000:], dtype=dtype)           # held-out rows land in their planted group's cluster
    hl, hs = held.assign(a.centroids)
    group_of = {int(t): int(l) for t, l in zip(truth[:1000].tolist(), a.labels.tolist())}
    assert hl.tolist() == [group_of[int(t)] for t in truth[1000:].tolist()]
    ref_a, ref_b, _ = R.assign_ref(held.features.cpu(), a.centroids.cpu())
    assert torch.equal(hl.cpu(), ref_a) and (hs.cpu().double() - ref_b).abs().max() <= R.assign_tol(128, held.features.cpu(), a.centroids.cpu())
    rep = a.representatives(3).cpu()
    lab, sc = a.labels.cpu(), a.scores.cpu()
    assert rep.shape == (8, 3) and rep.dtype == torch.int64
    for k in range(8):
        members = torch.nonzero(lab == k).flatten()
        order = sorted(members.tolist(), key=lambda r: (-sc[r].item(), r))
        assert rep[k].tolist() == (order + [-1, -1, -1])[:3]
    which, score = clip.name_clusters(a, init)                      # the prompts: the noisy directions the init was made of
    assert which.tolist() == [int(truth[:1000][lab == k][0]) for k in range(8)] and score.dtype == torch.float32
    purity, major = clip.cluster_purity(a.labels, truth[:1000])
    assert purity == 1.0 and major.tolist() == which.tolist()


def test_kmeans_errors():
    import clip
    feats = torch.randn(50, 64)
    with pytest.raises(ValueError, match="at least 1"):
        clip.kmeans(feats, 0)
    with pytest.raises(ValueError, match="above the 50 rows"):
        clip.kmeans(feats, 51)
    with pytest.raises(NotImplementedError, match="multiple of 32"):
        clip.kmeans(torch.randn(50, 40), 3)
    with pytest.raises(ValueError, match="empty"):
        clip.kmeans(clip.EmbeddingIndex(torch.zeros(0, 64)), 3)
    with pytest.raises(ValueError, match="init"):
        clip.kmeans(feats, 3, init="pca")
    with pytest.raises(ValueError, match="init must be"):
        clip.kmeans(feats, 3, init=torch.randn(4, 64))
    with pytest.raises(ValueError, match="empty"):
        clip.EmbeddingIndex(torch.zeros(0, 64)).assign(torch.randn(3, 64))
    with pytest.raises(ValueError, match="expected"):
        clip.EmbeddingIndex(feats).assign(torch.randn(3, 32))
    one = clip.kmeans(feats, 1)
    assert one.counts.tolist() == [50] and torch.isnan(one.margin).all() and one.converged and one.n_iter == 2


def test_cluster_images_script(tmp_path, capsys):
    import cluster_images
    from clip_caption.data import save_embeddings
    sizes = [30, 50, 20, 40]
    feats, truth, _ = R.planted(sizes, 64, 0.3, 77)
    names = ["fall", "machine", "shock", "gear"]
    caps, labelled = [], [0] * 4
    for i, t in enumerate(truth.tolist()):
        known = i % 3 == 0                                          # a third of the rows carries its type, the rest ''
        labelled[t] += known
        caps.append({"file_name": f"images/{names[t]}_{i:04d}.png", "clip_embedding": i, "caption": "", "violation_type": names[t] if known else ""})
    pkl, out = str(tmp_path / "emb.pkl"), str(tmp_path / "rows.json")
    save_embeddings(pkl, feats, caps)
    cluster_images.main(["--index", pkl, "--k", "4", "--show", "2", "--label-key", "violation_type", "--write-labels", out, "--n-init", "4"])
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    clusters, summary = lines[:-1], lines[-1]["summary"]
    assert len(clusters) == 4 and summary["rows"] == 140 and summary["k"] == 4 and summary["empty_clusters"] == 0 and summary["converged"]
    assert sorted(c["size"] for c in clusters) == sorted(sizes), "the planted sizes"
    for c in clusters:
        t = names.index(c["majority_label"])
        assert c["size"] == sizes[t] and c["majority_share"] == 1.0 and c["inherit"] == sizes[t] - labelled[t]
        assert len(c["representatives"]) == 2 and all(f"/{names[t]}_" in n for n in c["representatives"])
        assert 0.8 < c["concentration"] <= 1.001
    rows = json.load(open(out))
    assert len(rows) == 140 and [r["row"] for r in rows] == list(range(140))
    assert all(r["label"] == names[t] for r, t in zip(rows, truth.tolist()))
    assert sum(r["inherited"] for r in rows) == 140 - sum(labelled)
