"""clip.CacheClassifier on the MI355X, on the seeded fixture of cache_affinity_ref.py (9 centroids in 512 dimensions, 12 stored
rows per class, 90 queries, uninformative text features): the argmax against the float64 reference on every decided row,
leave_one_out against single-query calls, tune against a float64 sweep, the pickle round trip, add against a bulk build, and
scripts/fewshot_classify.py."""
import json
import os
import subprocess
import sys

import pytest
import torch

import cache_affinity_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return R.fewshot_fixture()


def _build(fx, dtype, **kw):
    import clip
    kw = dict(dict(text_features=fx["text"], alpha=R.FIX_ALPHA, beta=R.FIX_BETA, dtype=dtype), **kw)
    return clip.CacheClassifier(fx["features"], fx["labels"], **kw)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
def test_call_matches_float64_on_decided_rows(fx, dtype):
    clf = _build(fx, dtype)
    assert clf.num_classes == R.FIX_C and len(clf) == R.FIX_C * R.FIX_SHOTS
    assert torch.isnan(clf._laid.float()).all(dim=1).sum().item() == clf._laid.shape[0] - len(clf), "padding rows must be NaN"
    probs, idx, labels = clf(image_features=fx["queries"])                       # a host tensor: moved as EmbeddingIndex.search does
    assert probs.is_cuda and probs.shape == (R.FIX_Q, R.FIX_C) and labels == idx.tolist()
    assert torch.allclose(probs.sum(dim=1), torch.ones(R.FIX_Q, device="cuda"), atol=1e-5)
    q16, g16 = clf._queries(fx["queries"]).cpu(), clf.features.cpu()             # the 16-bit rows the kernel saw
    ref, tol = R.reference_logits(q16, g16, fx["labels"], R.FIX_C, R.FIX_ALPHA, R.FIX_BETA, text=fx["text"])
    got = clf.logits(fx["queries"]).cpu()
    print(f"[fewshot] {dtype} logits err/tol {((got.double() - ref).abs() / tol).max().item():.3e}")
    assert ((got.double() - ref).abs() <= tol).all()
    ok, top = R.decided(ref, tol)
    assert (~ok).double().mean().item() <= 0.01
    assert torch.equal(idx.cpu()[ok], top[ok])
    acc = (idx.cpu() == fx["query_labels"]).double().mean().item()
    zs = _build(fx, dtype, alpha=0.0)(image_features=fx["queries"])[1].cpu()     # the zero-shot term alone
    acc_zs = (zs == fx["query_labels"]).double().mean().item()
    print(f"[fewshot] {dtype} accuracy {acc:.3f}, zero-shot alone {acc_zs:.3f}")
    assert acc >= 0.95 and acc_zs <= 0.4
    named = _build(fx, dtype, class_names=[f"c{i}" for i in range(R.FIX_C)])
    assert named(image_features=fx["queries"].cuda())[2] == [f"c{i}" for i in idx.tolist()]
    import clip
    cm = clip.confusion_matrix(idx, fx["query_labels"], R.FIX_C)
    assert cm.is_cuda and cm.sum().item() == R.FIX_Q and cm.diag().sum().item() == round(acc * R.FIX_Q)


@pytest.mark.parametrize("per_class", ["sum", "mean"])
def test_leave_one_out_equals_single_queries(fx, per_class):
    clf = _build(fx, torch.bfloat16, per_class=per_class)
    loo = clf.leave_one_out()
    N = len(clf)
    assert loo.shape == (N, R.FIX_C)
    for i in range(N):
        one = clf.logits(fx["features"][i:i + 1], exclude=[i])
        assert torch.equal(one[0].view(torch.int32), loo[i].view(torch.int32)), f"row {i}"
    ref, tol = R.reference_logits(clf.features.cpu(), clf.features.cpu(), fx["labels"], R.FIX_C, R.FIX_ALPHA, R.FIX_BETA,
                                  text=fx["text"], exclude=torch.arange(N))
    if per_class == "sum":
        assert ((loo.cpu().double() - ref).abs() <= tol).all()
    # without the exclusion every row would meet itself at s = 1
    assert (clf.logits(fx["features"]) - loo).max().item() > 0.5 * R.FIX_ALPHA / (R.FIX_SHOTS if per_class == "mean" else 1)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=["bf16", "fp16"])
def test_tune_picks_the_float64_grid_point(fx, dtype):
    clf = _build(fx, dtype)
    alphas, betas = [0.0, 1.0, 20.0, 50.0], [1.0, 5.5]
    g16 = clf.features.cpu()
    q16 = clf._queries(fx["queries"]).cpu()
    for val in (False, True):
        # float64 sweep: per grid point the correct rows, and how many rows the reference leaves undecided (top-2 margin
        # within tol; at small alpha the noise of the text term decides some rows by less than fp32 can promise)
        want = torch.empty(len(alphas), len(betas), dtype=torch.float64)
        lo, hi = torch.empty_like(want), torch.empty_like(want)
        for i, al in enumerate(alphas):
            for j, be in enumerate(betas):
                if val:
                    ref, tol = R.reference_logits(q16, g16, fx["labels"], R.FIX_C, al, be, text=fx["text"])
                    target = fx["query_labels"]
                else:
                    ref, tol = R.reference_logits(g16, g16, fx["labels"], R.FIX_C, al, be, text=fx["text"], exclude=torch.arange(len(clf)))
                    target = fx["labels"]
                ok, top = R.decided(ref, tol)
                n = target.numel()
                want[i, j] = (top == target).double().sum() / n
                lo[i, j] = (ok & (top == target)).double().sum() / n
                hi[i, j] = lo[i, j] + (~ok).double().sum() / n
        first = int(want.reshape(-1).argmax())                                   # ties go to the first grid point
        flo, fhi = lo.reshape(-1), hi.reshape(-1)
        assert (fhi[:first] < flo[first]).all() and (fhi[first + 1:] <= flo[first]).all(), "the fixture's best grid point is not robust"
        a, b, acc, grid = clf.tune(alphas, betas, *((fx["queries"], fx["query_labels"]) if val else ()))
        print(f"[fewshot-tune] {dtype} val={val} picked alpha {a} beta {b} accuracy {acc:.3f}; undecided rows per point "
              f"{((hi - lo) * n).round().long().reshape(-1).tolist()}")
        assert grid.shape == want.shape and ((grid >= lo - 1e-12) & (grid <= hi + 1e-12)).all(), "an accuracy outside the reference's range"
        assert torch.equal(grid[hi == lo], want[hi == lo])
        assert (a, b) == (alphas[first // len(betas)], betas[first % len(betas)]) and acc == grid.reshape(-1)[first].item()


def test_pickle_round_trip_and_add(fx, tmp_path):
    import clip
    from clip_caption.data import save_embeddings
    names = ["fall", "gear", "site", "carry", "blast", "shock", "machine", "material", "puncture"]
    captions = [{"file_name": f"{i}.png", "violation_type": names[c], "clip_embedding": i} for i, c in enumerate(fx["labels"].tolist())]
    path = str(tmp_path / "support.pkl")
    save_embeddings(path, fx["features"], captions)
    clf = clip.CacheClassifier.from_pickle(path, "violation_type", class_names=names, beta=R.FIX_BETA)
    direct = clip.CacheClassifier(fx["features"], fx["labels"], class_names=names, beta=R.FIX_BETA)
    assert clf.class_names == names and torch.equal(clf.labels, fx["labels"])
    assert torch.equal(clf._laid.view(torch.int16), direct._laid.view(torch.int16))
    assert torch.equal(clf.affinity(fx["queries"]), direct.affinity(fx["queries"]))
    first = clip.CacheClassifier.from_pickle(path, "violation_type")              # order of first appearance
    assert first.class_names == list(dict.fromkeys(names[c] for c in fx["labels"].tolist()))
    assert clf(image_features=fx["queries"])[2] == first(image_features=fx["queries"])[2]
    # add equals a bulk build, bitwise
    n = 40
    grown = clip.CacheClassifier(fx["features"][:n], fx["labels"][:n], num_classes=R.FIX_C, beta=R.FIX_BETA)
    grown.add(fx["features"][n:70], fx["labels"][n:70]).add(fx["features"][70:].cuda(), fx["labels"][70:])
    assert len(grown) == len(direct) and torch.equal(grown.class_off, direct.class_off) and torch.equal(grown.class_len, direct.class_len)
    assert torch.equal(grown._laid.view(torch.int16), direct._laid.view(torch.int16))
    assert torch.equal(grown.affinity(fx["queries"]).view(torch.int32), direct.affinity(fx["queries"]).view(torch.int32))
    assert torch.equal(grown.leave_one_out().view(torch.int32), direct.leave_one_out().view(torch.int32))


def test_fewshot_script_synthetic():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fewshot_classify.py"), "--synthetic", "--tune"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert rows[0]["tuned"] is True and 0.0 <= rows[0]["leave_one_out_accuracy"] <= 1.0 and len(rows[0]["classes"]) == 9
    assert len(rows) == 1 + 27
    for row in rows[1:]:
        assert row["predicted"] in rows[0]["classes"] and row["file_name"].endswith(".png")
        assert abs(sum(row["probabilities"].values()) - 1.0) < 1e-3
