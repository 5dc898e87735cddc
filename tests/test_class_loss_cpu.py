"""CPU: the class-aware contrastive loss of clip/loss.py (labels= / text_labels=) against a float64 evaluation of its
definition (class_loss_helpers.ref_loss: soft-target cross-entropy, gradients by autograd) - square, rectangular, with
unlabelled rows and columns, with a non-unit upstream gradient, and data-parallel over gloo (world 2, classes spanning both
ranks) against the single-process evaluation on the concatenated batch.  The HIP launchers are replaced by
class_loss_helpers.ops_shim (torch restatements of their contracts); what is under test is the choreography of clip/loss.py,
plus class_ids / unique_texts and the declaration of the new launcher.  The kernel itself: tests/test_class_loss_gpu.py."""
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import class_loss_helpers as H  # noqa: E402


@pytest.fixture
def closs():
    import clip.loss as closs
    old = closs.ops
    closs.ops = H.ops_shim
    try:
        yield closs
    finally:
        closs.ops = old


def test_launcher_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+cclip_xent_rows_classes\s*\(", code)
    assert re.search(r"#define\s+CCLIP_ABI_VERSION\s+3\b", hdr)               # additive: the ABI version does not move
    from cclip_hip import ops
    assert callable(ops.xent_rows_classes)
    import clip
    assert callable(clip.class_ids) and callable(clip.unique_texts)


def _check(closs, N, M, E, a, b, seed, upstream=1.0, ls0=1.3, square_call=False):
    g = torch.Generator().manual_seed(seed)
    fi = torch.randn(N, E, generator=g).requires_grad_(True)
    ft = torch.randn(M, E, generator=g).requires_grad_(True)
    ls = torch.tensor(ls0, requires_grad=True)
    if square_call:
        loss, stats = closs.contrastive_loss(fi, ft, ls, labels=a)
    else:
        loss, stats = closs.contrastive_loss(fi, ft, ls, labels=a, text_labels=b)
    (loss * upstream).backward()
    ref, correct, dfi, dft, dls = H.ref_loss_and_grads(fi, ft, ls, a, b, upstream)
    print(f"N={N} M={M}: loss {loss.item():.7f} ref {ref.item():.7f} | rel dfi {H.rel(fi.grad, dfi):.2e} dft {H.rel(ft.grad, dft):.2e}"
          f" | dls {ls.grad.item():.6e} ref {dls.item():.6e} | correct {int(stats[1])} ref {correct}")
    assert abs(loss.item() - ref.item()) < H.LOSS_TOL and abs(stats[0].item() - ref.item()) < H.LOSS_TOL
    assert int(stats[1].item()) == correct and stats.shape == (2,)
    assert H.rel(fi.grad, dfi) < H.GRAD_TOL and H.rel(ft.grad, dft) < H.GRAD_TOL
    assert H.scalar_close(ls.grad, dls)
    return fi, ft


def test_square_three_classes(closs):
    a = torch.tensor([0, 1, 2, 0, 1, 2, 2, 2, 0, 1, 0, 0])
    _check(closs, 12, 12, 16, a, a, seed=1, square_call=True)
    _check(closs, 12, 12, 16, a.to(torch.int32), a.to(torch.int32), seed=2, square_call=True)      # int32 labels too


def test_rectangular_37_by_9(closs):
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 9, (37,), generator=g)
    _check(closs, 37, 9, 16, a, torch.arange(9), seed=4)


def test_unlabelled_rows_and_columns(closs):
    a = torch.tensor([0, -1, 2, 0, 1, -1, 2, 3, 0, 1, -1, 0])               # class 3 has no text: a row without positives
    b = torch.tensor([0, 1, -1, 2, -1, 1, 4])                               # class 4 has no image; two unlabelled columns
    fi, ft = _check(closs, 12, 7, 16, a, b, seed=5)
    # with every image row unlabelled no row or column has a positive: nothing is left on either side
    ls = torch.tensor(1.0, requires_grad=True)
    none = torch.full((12,), -1)
    loss, stats = closs.contrastive_loss(fi.detach().requires_grad_(True), ft.detach().requires_grad_(True), ls, labels=none, text_labels=b)
    loss.backward()
    assert loss.item() == 0.0 and stats[1].item() == 0.0 and ls.grad.item() == 0.0


def test_non_unit_upstream_gradient(closs):
    a = torch.tensor([0, 1, 2, 0, 1, 2, 2, 2, 0, 1, 0, 0])
    _check(closs, 12, 12, 16, a, a, seed=6, upstream=2.5, square_call=True)
    _check(closs, 12, 5, 16, a, torch.tensor([2, 0, 1, 0, -1]), seed=7, upstream=-0.75)


def test_arange_labels_equal_the_pairwise_path(closs):
    g = torch.Generator().manual_seed(8)
    N, E = 12, 16
    fi0, ft0 = torch.randn(N, E, generator=g), torch.randn(N, E, generator=g)
    res = []
    for labels in (None, torch.arange(N)):
        fi, ft, ls = fi0.clone().requires_grad_(True), ft0.clone().requires_grad_(True), torch.tensor(2.0, requires_grad=True)
        loss, stats = closs.contrastive_loss(fi, ft, ls, labels=labels)
        loss.backward()
        res.append((loss.detach(), stats, fi.grad, ft.grad, ls.grad))
    (l0, s0, a0, b0, c0), (l1, s1, a1, b1, c1) = res
    assert abs(l0.item() - l1.item()) < H.LOSS_TOL and s0[1].item() == s1[1].item()
    assert H.rel(a1, a0) < H.GRAD_TOL and H.rel(b1, b0) < H.GRAD_TOL and H.scalar_close(c1, c0)


def test_argument_errors(closs):
    fi, ft, ls = torch.randn(4, 8), torch.randn(4, 8), torch.tensor(1.0)
    with pytest.raises(TypeError):
        closs.contrastive_loss(fi, ft, ls, labels=torch.zeros(4))                          # float class ids
    with pytest.raises(ValueError):
        closs.contrastive_loss(fi, ft, ls, labels=torch.zeros(3, dtype=torch.int64))       # one id per row
    with pytest.raises(ValueError):
        closs.contrastive_loss(fi, ft[:3], ls, labels=torch.zeros(4, dtype=torch.int64))   # square form needs N == M
    with pytest.raises(ValueError):
        closs.contrastive_loss(fi, ft, ls, text_labels=torch.zeros(4, dtype=torch.int64))  # text_labels without labels


def test_class_ids_and_unique_texts_single_process():
    import clip
    g = torch.Generator().manual_seed(9)
    base = torch.randint(1, 1000, (5, 77), generator=g, dtype=torch.int32)
    pick = torch.tensor([3, 0, 3, 4, 1, 0, 0, 2, 4, 3, 1])
    tokens = base[pick]
    ids = clip.class_ids(tokens)
    assert ids.dtype == torch.int32 and ids.shape == (11,)
    assert torch.equal(ids[:, None] == ids[None, :], pick[:, None] == pick[None, :])      # equal ids exactly for equal rows
    uniq, inverse = clip.unique_texts(tokens)
    assert inverse.dtype == torch.int32 and uniq.shape == (5, 77) and uniq.dtype == tokens.dtype
    assert torch.equal(uniq[inverse.long()], tokens)


# ---- gloo, world 2 ---------------------------------------------------------------------------------------------------------
_N, _E = 12, 16
_CLASSES = [0, 1, 2, 0, 1, -1, 2, 2, 0, 3, 1, 0]          # every class but 3 has rows on rank 0 (rows 0-5) AND rank 1 (rows 6-11)


def _dp_inputs():
    g = torch.Generator().manual_seed(321)
    fi, ft = torch.randn(_N, _E, generator=g), torch.randn(_N, _E, generator=g)
    base = torch.randint(1, 1000, (5, 77), generator=g, dtype=torch.int32)
    return fi, ft, torch.tensor(1.3), torch.tensor(_CLASSES), base


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "construction-clip_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import clip.loss as closs
    import clip.parallel as par
    import class_loss_helpers as helpers
    closs.ops = helpers.ops_shim
    par.init_distributed("gloo")
    fi_all, ft_all, ls, classes, base = _dp_inputs()
    nloc = _N // world
    sl = slice(rank * nloc, (rank + 1) * nloc)
    # rectangular + live group: refused BEFORE any collective (rank 1 never calls it: were a collective issued, rank 0 would hang
    # in it and the join below would time out instead of passing)
    refused = True
    if rank == 0:
        try:
            closs.contrastive_loss(fi_all[sl], ft_all[sl], ls, labels=classes[sl], text_labels=classes[sl])
            refused = False
        except NotImplementedError:
            pass
    fi, ft = fi_all[sl].clone().requires_grad_(True), ft_all[sl].clone().requires_grad_(True)
    lsp = ls.clone().requires_grad_(True)
    loss, stats = closs.ContrastiveLoss()(fi, ft, lsp, labels=classes[sl])
    (loss * 2.0).backward()                        # non-unit upstream gradient
    # class ids of token rows: the classes (shifted: -1 -> row 0 of `base`) pick the rows, so equal class <=> equal row
    tokens = base[(classes + 1).clamp(max=4)]
    ids = closs.class_ids(tokens[sl])
    torch.save(dict(loss=loss.detach(), stats=stats, dfi=fi.grad, dft=ft.grad, dls=lsp.grad, refused=refused, ids=ids),
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_dp_class_aware_matches_single_process(tmp_path):
    world, port = 2, 30000 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    fi, ft, ls, classes, base = _dp_inputs()
    ref, correct, dfi, dft, dls = H.ref_loss_and_grads(fi, ft, ls, classes, classes, upstream=2.0)
    outs = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(world)]
    nloc = _N // world
    for r, o in enumerate(outs):
        assert o["refused"]
        assert abs(o["loss"].item() - ref.item()) < H.LOSS_TOL                  # every rank reports the GLOBAL loss
        assert int(o["stats"][1].item()) == correct                            # global #correct, by class
        assert H.rel(o["dfi"], dfi[r * nloc:(r + 1) * nloc]) < H.GRAD_TOL
        assert H.rel(o["dft"], dft[r * nloc:(r + 1) * nloc]) < H.GRAD_TOL
    assert H.scalar_close(sum(o["dls"] for o in outs), dls)                    # SUM over ranks, as allreduce_gradients does
    # class_ids: one numbering on both ranks - equal ids exactly for equal token rows, across the rank boundary too
    ids = torch.cat([o["ids"] for o in outs])
    rows = (classes + 1).clamp(max=4)
    assert ids.dtype == torch.int32 and torch.equal(ids[:, None] == ids[None, :], rows[:, None] == rows[None, :])
