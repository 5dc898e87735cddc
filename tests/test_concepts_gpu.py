"""GPU: clip.decompose / EmbeddingIndex.decompose end to end - against the CPU stand-in path on the same rows, planted
recovery through the public API, `recompose` against the `cosine` read-out, and scripts/explain_concepts.py --synthetic."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import concepts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def test_decompose_matches_the_stand_in_path_and_chunks_are_bitwise():
    import clip
    import concepts_ops_shim as shim
    x16, c16, _ = R.planted(200, 64, 40, seed=1)
    d = clip.ConceptDictionary(c16.cuda(), names=[f"w{v}" for v in range(200)])
    index = clip.EmbeddingIndex(x16.float())
    x16 = index.features.cpu()                                 # the rows as stored
    dec = index.decompose(d, l1=0.05, iters=100)
    w, _, _, nnz, _, kkt = shim.concept_codes(x16, c16, 0.05, 1.0 / d.L, 100)
    top, at = torch.topk(w, 32, dim=1)
    # fp32 restatement against the kernel: the kernel tests' float64 tolerance on either side
    assert (dec.weights.cpu() - top.clamp(min=0)).abs().max() <= 2 * 4 * 2.06e-6
    strong = top > 1e-3
    assert torch.equal(dec.indices.cpu()[strong], at[strong])
    chunked = clip.decompose(index, d, l1=0.05, iters=100, chunk_bytes=8 * 200 * 7)
    for k in ("indices", "weights", "nnz", "cosine", "kkt", "delta", "l1norm", "resid2", "truncated"):
        assert torch.equal(getattr(dec, k), getattr(chunked, k)), k
    assert dec.terms(0)[0][0].startswith("w") and len(dec) == 40


@pytest.mark.parametrize("V,D", [(75, 32), (1000, 512)])
def test_planted_pairs_through_the_public_api(V, D):
    import clip
    x16, c16, pairs = R.planted(V, D, 16, seed=V + D)
    d = clip.ConceptDictionary(c16.cuda())
    dec = clip.decompose(x16.cuda(), d, l1=0.1, iters=200)
    for i in range(16):
        got = set(dec.indices[i][dec.weights[i] > 1e-3].tolist())
        assert got == set(pairs[i].tolist()), (i, got, pairs[i])
    assert (dec.nnz == 2).all() and not dec.truncated.any()


def test_recompose_agrees_with_the_cosine_readout():
    import clip
    x16, c16 = R.unit_rows16(50, 64, 3, torch.bfloat16), R.unit_rows16(300, 64, 4, torch.bfloat16)
    d = clip.ConceptDictionary(c16.cuda())
    dec = clip.decompose(x16.cuda(), d, l1=0.05, iters=100, max_terms=64)
    back = dec.recompose()
    cos = (back * torch.nn.functional.normalize(x16.cuda().float(), dim=1)).sum(1)
    assert (cos - dec.cosine).abs().max() <= 4 * 2.0 ** -24    # the same fp32 expression, evaluated twice
    # cosine^2 = 1 - resid2 of the best scaling <= the kernel's resid2 at its own scaling: |x|^2 (1 - cos^2) <= resid2
    xx = (x16.cuda().float() ** 2).sum(1)
    full = ~dec.truncated
    assert (xx * (1 - dec.cosine ** 2))[full].le(dec.resid2[full] + 1e-5).all()
    centred = clip.decompose(x16.cuda(), clip.ConceptDictionary(c16.cuda().float(), center="mean"), l1=0.05, iters=50, center="mean")
    assert centred.recompose().shape == (50, 64) and torch.isfinite(centred.cosine).all()


def test_script_synthetic(capsys):
    """scripts/explain_concepts.py --synthetic: what it prints is what it returns, one line per photo, one per group and a
    summary; the concepts it names are those of the float64 reference on the same 16-bit rows."""
    import json
    import numpy as np
    import clip
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import explain_concepts as M
    import _common as C
    lines, groups, summary, dec = M.main(["--synthetic", "--top", "4"])
    printed = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert printed == lines + groups + [dict(summary=summary)]
    V = len(C.CLASSES) + len(M.SYNTHETIC_WORDS)
    assert summary["rows"] == len(lines) == 54 and summary["vocabulary"] == V and summary["groups"] == len(groups) == 9
    assert summary["centred"] and summary["iters"] == 200 and summary["truncated"] == 0
    for r, ln in enumerate(lines):
        assert set(ln) == {"row", "file_name", "concepts", "cosine", "nnz", "kkt"} and ln["row"] == r
        ws = [w for _, w in ln["concepts"]]
        assert 1 <= len(ws) <= 4 and ws == sorted(ws, reverse=True) and min(ws) > 0 and ln["nnz"] >= len(ws)
        assert 0.0 < ln["cosine"] <= 1.0 + 1e-6 and 0.0 <= ln["kkt"] < float("inf")
    # the float64 recurrence on the rows and the dictionary the script used
    feats, caps, _ = M.synthetic_pickle(dec.dictionary)
    assert [c["file_name"] for c in caps] == [ln["file_name"] for ln in lines]
    x16 = clip.EmbeddingIndex(feats, dtype=torch.bfloat16).features.cpu()
    ref = R.fista64(R.rows64(x16), R.rows64(dec.dictionary.rows.cpu()), 0.1, np.float32(1.0 / dec.dictionary.L), 200)["w"]
    names = dec.dictionary.names
    # 1e-3 is a thousand kernel tolerances: a difference that size is a different answer, whatever the conditioning of this
    # dictionary; a top concept is compared where the reference's own first two lie further apart than that
    for r, ln in enumerate(lines):
        order = np.argsort(-ref[r])
        for name, w in ln["concepts"]:
            assert abs(w - ref[r, names.index(name)]) < 1e-3, (r, name)
        if ref[r, order[0]] - ref[r, order[1]] > 1e-3:
            assert ln["concepts"][0][0] == names[order[0]], (r, ln["concepts"], names[order[0]])
        assert ln["nnz"] >= int((ref[r] > 1e-3).sum())
    cls = np.array([C.CLASSES.index(c["violation_type"]) for c in caps])
    assert [g["group"] for g in groups] == sorted(C.CLASSES) and all(g["size"] == 6 for g in groups)
    for g in groups:
        excess = ref[cls == C.CLASSES.index(g["group"])].mean(0) - ref.mean(0)
        order = np.argsort(-excess)
        assert len(g["distinctive"]) == 4 and g["top"] and abs(g["distinctive"][0][1] - excess[order[0]]) < 1e-3
        if excess[order[0]] - excess[order[1]] > 1e-3:
            assert g["distinctive"][0][0] == names[order[0]], (g, names[order[0]])
