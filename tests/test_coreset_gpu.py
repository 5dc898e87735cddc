"""clip.select_coreset and EmbeddingIndex.coreset end to end on the MI355X, against the float64 replay of
tests/coreset_ref.py: planted clusters whose picks must equal the reference's exactly (the separation is verified on the host in
tests/test_coreset_cpu.py), noisy clusters that touch (every pick and every owner inside the derived bounds, no row left out),
seeds, weights, the full selection, bitwise repeatability, the counts and one run of scripts/select_to_label.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreset_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = (torch.bfloat16, torch.float16)
IDS = ["bf16", "fp16"]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def replay(X, res, w=None, seeds=(), first=None):
    return R.check_selection(X, w, res.picks.cpu().numpy(), res.radius.cpu().numpy(), res.distance.double().cpu().numpy(),
                             res.owner.cpu().numpy(), seeds=seeds, first=first)


def mean_row(X):
    mean = X.sum(0)
    return R.argmax_key(X @ (mean / np.linalg.norm(mean)), np.ones(len(X), dtype=bool))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_planted_clusters_one_pick_each_exactly(dtype):
    import clip
    P = R.PLANTED
    x16, cls = R.planted_clusters16(dtype=dtype, **P)
    X = R.rows64(x16)
    res = clip.select_coreset(x16.cuda(), P["K"])
    ref = R.greedy(X, None, P["K"], first=mean_row(X))
    picks = res.picks.cpu().numpy()
    bad, ratio = replay(X, res)
    print(f"[coreset] planted {dtype}: largest err / tol = {ratio:.4f}")
    assert np.array_equal(picks, ref["picks"])
    assert sorted(cls[picks]) == list(range(P["K"])) and not bad, bad
    assert res.radius[0].item() == float("inf") and (res.radius[1:].diff() <= 0).all()
    assert (cls[res.owner.cpu().numpy()] == cls).all()                     # every row sits under its own cluster's pick
    assert abs(res.cover_radius.item() - ref["mind"].max()) <= ref["tol"].max()


@pytest.mark.parametrize("D,noise", [(64, 1.2), (512, 1.5)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_noisy_clusters_every_pick_and_owner(dtype, D, noise):
    import clip
    x16, _ = R.planted_clusters16(K=5, per=80, D=D, noise=noise, seed=D, dtype=dtype)
    index = clip.EmbeddingIndex(x16.float(), dtype=dtype)
    X = R.rows64(index.features)
    res = index.coreset(60)
    bad, ratio = replay(X, res)
    print(f"[coreset] noisy D={D} {dtype}: largest err / tol = {ratio:.4f}")
    assert not bad, bad
    assert res.picks[0].item() == mean_row(X) and res.picks.unique().numel() == 60
    again = clip.select_coreset(index, 60)                                 # two fresh calls are bitwise equal
    assert torch.equal(again.picks, res.picks) and same_bits(again.radius, res.radius)
    assert same_bits(again.distance, res.distance) and torch.equal(again.owner, res.owner)
    centres, counts = res.cover_counts()
    assert torch.equal(centres, res.picks) and counts.sum().item() == 400
    assert torch.equal(counts, torch.bincount(res.owner, minlength=400)[centres])
    assert res.covered(2.0).item() == 1.0 and res.covered(-1.0).item() == 0.0
    assert res.covered(res.cover_radius.item()).item() == 1.0
    by_row = clip.select_coreset(index, 5, first=123)
    assert by_row.picks[0].item() == 123 and not replay(X, by_row, first=123)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_seeds(dtype):
    import clip
    K, per = 6, 40
    x16, cls = R.planted_clusters16(K=K, per=per, D=64, noise=0.5, seed=8, dtype=dtype)
    x = x16.cuda()
    X = R.rows64(x16)
    g = np.random.RandomState(0)
    labels = np.full(K * per, -1)
    for k in range(K - 1):                                                  # every cluster but the last carries three labels
        labels[g.choice(np.nonzero(cls == k)[0], 3, replace=False)] = k
    seeds = np.nonzero(labels >= 0)[0]
    res = clip.select_coreset(x, 30, labelled=torch.from_numpy(labels))
    picks = res.picks.cpu().numpy()
    assert not set(picks.tolist()) & set(seeds.tolist()) and len(set(picks.tolist())) == 30
    assert cls[picks[0]] == K - 1                                           # the unlabelled cluster is the farthest
    assert res.seeds.cpu().tolist() == seeds.tolist()
    bad, ratio = replay(X, res, seeds=seeds.tolist())
    print(f"[coreset] seeds {dtype}: largest err / tol = {ratio:.4f}")
    assert not bad, bad
    for form in (seeds.tolist(), torch.from_numpy(labels >= 0).cuda()):
        other = clip.select_coreset(x, 30, labelled=form)
        assert torch.equal(other.picks, res.picks) and same_bits(other.distance, res.distance)
    none = clip.select_coreset(x, 0, labelled=seeds.tolist())
    assert none.picks.numel() == 0 and set(none.owner.cpu().tolist()) == set(seeds.tolist())
    centres, counts = res.cover_counts()
    assert centres.numel() == len(seeds) + 30 and counts.sum().item() == K * per


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weights(dtype):
    import clip
    K, per = 6, 50
    x16, cls = R.planted_clusters16(K=K, per=per, D=64, noise=0.6, seed=5, dtype=dtype)
    index = clip.EmbeddingIndex(x16.float(), dtype=dtype)
    X = R.rows64(index.features)
    g = np.random.RandomState(1)
    w = g.uniform(0.2, 1.0, K * per).astype(np.float32)
    w[(cls == 2) | (cls == 4)] = 0.0                                        # a region that must never be picked
    w[np.nonzero(cls == 0)[0][:3]] = np.nan
    res = index.coreset(80, weights=torch.from_numpy(w))
    picks = res.picks.cpu().numpy()
    assert (w[picks] > 0).all() and len(set(picks.tolist())) == 80
    # the first pick: the most similar to the mean among the 64 nearest rows that are eligible
    sim = X @ (X.sum(0) / np.linalg.norm(X.sum(0)))
    near = np.argsort(-sim, kind="stable")[:64]
    first = int(near[np.nonzero(w[near] > 0)[0][0]])
    assert sim[picks[0]] >= sim[first] - 4 * 64 * R.U - 2.0 ** -8       # (the device ranks against the mean rounded to 16 bits)
    first = int(picks[0])
    bad, ratio = replay(X, res, w=w.astype(np.float64), first=first)
    print(f"[coreset] weights {dtype}: largest err / tol = {ratio:.4f}")
    assert not bad, bad
    # 1 - certainty of a real spread_labels call, end to end, on clusters that overlap (separate ones are all certain: weight 0)
    x16, cls = R.planted_clusters16(K=K, per=per, D=64, noise=2.0, seed=6, dtype=dtype)
    index = clip.EmbeddingIndex(x16.float(), dtype=dtype)
    X = R.rows64(index.features)
    labels = np.full(K * per, -1)
    for k in range(K):
        labels[np.nonzero(cls == k)[0][:2]] = k
    spread = index.spread_labels(torch.from_numpy(labels), n_classes=K, k=10)
    unsure = 1.0 - spread.certainty
    res = index.coreset(40, labelled=torch.from_numpy(labels), weights=unsure)
    seeds = np.nonzero(labels >= 0)[0].tolist()
    bad, ratio = replay(X, res, w=unsure.double().cpu().numpy(), seeds=seeds)
    print(f"[coreset] 1 - certainty {dtype}: largest err / tol = {ratio:.4f}")
    assert not bad, bad
    live = res.picks[res.picks >= 0].cpu().tolist()
    assert len(live) and not set(live) & set(seeds) and (unsure[live] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_row_ends_as_a_centre(dtype):
    import clip
    x16 = R.unit_rows16(300, 96, 4, dtype)
    seeds = [0, 150, 299]
    res = clip.select_coreset(x16.cuda(), 297, labelled=seeds)
    assert sorted(res.picks.cpu().tolist() + seeds) == list(range(300))
    assert (res.distance == 0).all() and torch.equal(res.owner.cpu(), torch.arange(300))
    assert res.cover_radius.item() == 0.0 and res.cover_counts()[1].sum().item() == 300
    with pytest.raises(ValueError):
        clip.select_coreset(x16.cuda(), 298, labelled=seeds)


def test_script_on_a_synthetic_pickle(tmp_path, capsys):
    import select_to_label as M
    import _common as C
    from clip_caption.data import save_embeddings
    x16, cls = R.planted_clusters16(K=9, per=30, D=64, noise=0.6, seed=2, dtype=torch.bfloat16)
    known = np.zeros(270, dtype=bool)
    for k in range(8):
        known[np.nonzero(cls == k)[0][:4]] = True
    caps = [{"file_name": f"images/{i:04d}.png", "clip_embedding": i, "violation_type": C.CLASSES[int(cls[i])] if known[i] else ""}
            for i in range(270)]
    pkl = str(tmp_path / "e.pkl")
    save_embeddings(pkl, x16.float(), caps)
    for extra, m in ((["--label-key", "violation_type"], 20), (["--label-key", "violation_type", "--uncertainty", "--k", "10"], 15), ([], 12)):
        lines, summary = M.main(["--index", pkl, "--m", str(m)] + extra)
        printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(lines) == m and len(printed) == m + 1 and printed[:m] == lines and printed[-1] == dict(summary=summary)
        assert all(set(ln) == {"rank", "row", "file_name", "radius", "covers"} for ln in lines)
        assert [ln["rank"] for ln in lines] == list(range(m)) and len({ln["row"] for ln in lines}) == m
        assert all(ln["file_name"] == caps[ln["row"]]["file_name"] and ln["covers"] >= 1 for ln in lines)
        if extra:
            assert not any(known[ln["row"]] for ln in lines) and summary["labelled"] == 32
            assert all(isinstance(ln["radius"], float) for ln in lines)
            assert cls[lines[0]["row"]] == 8 or "--uncertainty" in extra        # the cluster without a label is the farthest
        else:
            assert lines[0]["radius"] is None and summary["labelled"] == 0
    lines, summary = M.main(["--synthetic", "--m", "7"])
    capsys.readouterr()
    assert len(lines) == 7 and summary["picked"] == 7 and summary["labelled"] > 0
