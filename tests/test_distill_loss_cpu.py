"""CPU: the distillation loss of clip/loss.py (distill_loss, DistillLoss) against a float64 evaluation of its definition
(distill_loss_helpers.ref_loss: kl_div over log_softmax of the scaled cosines, both directions, gradients by autograd) - square,
rectangular and with a teacher of another embedding width; its invariants (a detached teacher, zero at teacher == student,
gradient rows that sum to zero); the refusals; the declaration and export of cclip_kl_rows; and the new options of
scripts/train_clip.py.  The HIP launchers are replaced by distill_loss_helpers.ops_shim (torch restatements of their contracts):
what is under test here is the choreography.  The kernel itself: tests/test_distill_loss_kernels_gpu.py."""
import os
import re
import sys
import types

import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import distill_loss_helpers as H  # noqa: E402


@pytest.fixture
def closs():
    import clip.loss as closs
    old = closs.ops
    closs.ops = H.ops_shim
    try:
        yield closs
    finally:
        closs.ops = old


# ---- the reference itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,C,scale", [(5, 7, 1.0), (3, 70, 10.0), (4, 1, 1.0), (6, 33, 100.0)])
def test_reference_rows_against_kl_div(R, C, scale):
    g = torch.Generator().manual_seed(R * 100 + C)
    L = (torch.randn(R, C, generator=g, dtype=torch.float64) * scale).requires_grad_(True)
    G = torch.randn(R, C, generator=g, dtype=torch.float64) * scale
    gs = 0.37
    loss_row, d, rowdot, pred, agree = H.ref_rows(L, G, gs)
    kl = torch.nn.functional.kl_div(torch.log_softmax(L, 1), torch.softmax(G, 1), reduction="none").sum(1)
    (kl.sum() * gs).backward()
    assert torch.allclose(loss_row, kl.detach(), rtol=1e-12, atol=1e-13)
    assert torch.allclose(d, L.grad, rtol=1e-12, atol=1e-15)
    assert torch.allclose(rowdot, (L.grad * L.detach()).sum(1), rtol=1e-12, atol=1e-12)
    assert torch.equal(pred, L.argmax(1)) and torch.equal(agree, L.argmax(1) == G.argmax(1))
    assert d.sum(1).abs().max().item() <= 1e-15 * C                          # both softmaxes sum to one
    assert bool((loss_row >= -1e-15).all())                                  # a KL divergence


def test_reference_and_shim_skip_a_teacher_cell_at_minus_infinity():
    g = torch.Generator().manual_seed(3)
    L, G = torch.randn(4, 9, generator=g), torch.randn(4, 9, generator=g)
    G[1, 4] = -float("inf")
    keep = [c for c in range(9) if c != 4]
    whole = H.ref_rows(L, G)[0]
    assert bool(torch.isfinite(whole).all())
    # the row without that column, the student's softmax still over all nine: the cell added exactly nothing
    a = G[1, keep].double() - torch.logsumexp(G[1, keep].double(), 0)
    b = L[1, keep].double() - torch.logsumexp(L[1].double(), 0)
    assert whole[1].item() == pytest.approx((a.exp() * (a - b)).sum().item(), rel=1e-13)
    loss_row = torch.empty(4)
    H.kl_rows(L, G, loss_row=loss_row)
    assert torch.allclose(loss_row.double(), whole, atol=1e-5)


# ---- choreography ----------------------------------------------------------------------------------------------------------
def _inputs(N, M, E, Et, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, E, generator=g), torch.randn(M, E, generator=g), torch.randn(N, Et, generator=g),
            torch.randn(M, Et, generator=g))


def _check(closs, N, M, E, Et, seed, ts=20.0, upstream=1.0, ls0=1.3):
    fi, ft, ti, tt = _inputs(N, M, E, Et, seed)
    fi.requires_grad_(True); ft.requires_grad_(True)
    ls = torch.tensor(ls0, requires_grad=True)
    loss, stats = closs.distill_loss(fi, ft, ls, ti, tt, ts)
    (loss * upstream).backward()
    ref, agree, dfi, dft, dls, abs_ls = H.ref_loss_and_grads(fi, ft, ls, ti, tt, ts, upstream)
    print(f"N={N} M={M} E={E} Et={Et}: loss {loss.item():.7f} ref {ref.item():.7f} | rel dfi {H.rel(fi.grad, dfi):.2e} "
          f"dft {H.rel(ft.grad, dft):.2e} | dls {ls.grad.item():.6e} ref {dls.item():.6e} | agree {int(stats[1])} ref {agree}")
    assert abs(loss.item() - ref.item()) <= H.LOSS_TOL and abs(stats[0].item() - ref.item()) <= H.LOSS_TOL
    assert stats.shape == (2,) and int(stats[1].item()) == agree and not stats.requires_grad
    assert H.rel(fi.grad, dfi) < H.GRAD_TOL and H.rel(ft.grad, dft) < H.GRAD_TOL
    assert H.sum_close(ls.grad, dls, abs_ls) and ls.grad.shape == ()
    assert fi.grad.shape == fi.shape and ft.grad.shape == ft.shape


def test_square_8(closs):
    _check(closs, 8, 8, 16, 16, seed=1)


def test_rectangular_8_by_5(closs):
    _check(closs, 8, 5, 16, 16, seed=2)


def test_teacher_of_another_width(closs):
    _check(closs, 8, 8, 16, 24, seed=3)
    _check(closs, 8, 5, 16, 12, seed=4, upstream=-0.75)                      # and a non-unit upstream gradient


def test_teacher_scale_as_a_tensor_and_the_module(closs):
    fi, ft, ti, tt = _inputs(8, 5, 16, 24, 5)
    ls = torch.tensor(1.3)
    as_float = closs.distill_loss(fi, ft, ls, ti, tt, 20.0)[0]
    as_tensor = closs.distill_loss(fi, ft, ls, ti, tt, torch.tensor(20.0))[0]
    # exp(log(20)) in fp32 is 20 within two roundings of 3.0: the teacher's logits move by <= 20 * 4e-7
    assert abs(as_float.item() - as_tensor.item()) <= 1e-5
    mod = closs.DistillLoss(torch.tensor(20.0))
    assert list(mod.parameters()) == [] and mod.teacher_scale.shape == () and mod.teacher_scale.dtype == torch.float32
    loss, stats = mod(fi, ft, ls, ti, tt)
    assert torch.equal(loss, as_tensor) and stats.shape == (2,)
    import clip
    assert clip.distill_loss is closs.distill_loss and clip.DistillLoss is closs.DistillLoss
    assert issubclass(clip.DistillLoss, torch.nn.Module)


# ---- invariants ------------------------------------------------------------------------------------------------------------
def test_teacher_tensors_receive_no_gradient(closs):
    fi, ft, ti, tt = (x.requires_grad_(True) for x in _inputs(8, 5, 16, 24, 6))
    ls = torch.tensor(1.3, requires_grad=True)
    ts = torch.tensor(20.0, requires_grad=True)
    loss, _ = closs.distill_loss(fi, ft, ls, ti, tt, ts)
    loss.backward()
    assert fi.grad is not None and ft.grad is not None and ls.grad is not None
    assert ti.grad is None and tt.grad is None and ts.grad is None
    # a student that asks for nothing: forward only, the same value
    with torch.no_grad():
        again, _ = closs.distill_loss(fi, ft, ls, ti, tt, ts)
    assert torch.equal(again, loss.detach())


def test_teacher_equal_to_student_is_zero(closs):
    fi, ft, _, _ = _inputs(8, 5, 16, 16, 7)
    fi.requires_grad_(True); ft.requires_grad_(True)
    ls = torch.tensor(1.3, requires_grad=True)
    loss, stats = closs.distill_loss(fi, ft, ls, fi.detach().clone(), ft.detach().clone(), ls.detach().exp())
    loss.backward()
    # student and teacher logits (|L| <= e^1.3 < 4) differ by the rounding of the scale alone, d <= 4 ulp(4) = 1e-6: the KL is
    # second order in d, a logits gradient row is <= 2 d / 2N in sum, and a feature gradient <= s times that over the rows
    assert 0.0 <= loss.item() <= 1e-10 and int(stats[1].item()) == 8
    assert fi.grad.abs().max().item() <= 1e-5 and ft.grad.abs().max().item() <= 1e-5 and abs(ls.grad.item()) <= 1e-5


def test_every_logits_gradient_row_sums_to_zero(closs):
    seen = []
    real = H.ops_shim.kl_rows

    def spy(logits, teacher, **kw):
        real(logits, teacher, **kw)
        seen.append((kw["dlogits"].clone(), kw["dlogits"] is logits, kw["grad_scale"]))

    closs.ops = types.SimpleNamespace(**{**vars(H.ops_shim), "kl_rows": spy})
    fi, ft, ti, tt = _inputs(8, 5, 16, 24, 8)
    fi.requires_grad_(True)
    closs.distill_loss(fi, ft, torch.tensor(1.3), ti, tt, 20.0)[0].backward()
    assert [tuple(d.shape) for d, _, _ in seen] == [(8, 5), (5, 8)]
    assert [gs for _, _, gs in seen] == [1 / 16, 1 / 10]                     # 1 / 2N and 1 / 2M
    for d, in_place, gs in seen:
        assert in_place                                                      # the gradient overwrites the student's logits
        assert d.abs().sum().item() > 0
        assert d.sum(1).abs().max().item() <= 4 * 6e-8 * gs * d.shape[1]     # two softmaxes that each sum to one, in fp32


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_argument_errors(closs):
    fi, ft, ti, tt = _inputs(8, 5, 16, 24, 9)
    ls = torch.tensor(1.0)
    with pytest.raises(ValueError, match="teacher_image_features"):
        closs.distill_loss(fi, ft, ls, ti[:7], tt, 20.0)                     # one teacher row per student row
    with pytest.raises(ValueError, match="teacher_text_features"):
        closs.distill_loss(fi, ft, ls, ti, tt[:4], 20.0)
    with pytest.raises(ValueError):
        closs.distill_loss(fi, ft, ls, ti, tt[:, :20], 20.0)                 # one width per model
    with pytest.raises(ValueError):
        closs.distill_loss(fi, ft, ls, ti, tt, torch.ones(2))                # a scalar scale


def test_binding_refuses_before_any_launch():
    from cclip_hip import ops
    lg, te = torch.randn(4, 9), torch.randn(4, 9)
    with pytest.raises(TypeError, match="logits"):
        ops.kl_rows(lg, te)                                                  # CPU tensors


def test_binding_checks_the_teacher(monkeypatch):
    """the shared argument check past its device test (there is no device here): dtype, shape, stride and device of `teacher`
    and of the per-row outputs; every call below must raise before the library is reached"""
    from cclip_hip import ops

    def dtype_only(t, dtype, name):
        if t.dtype != dtype:
            raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")

    monkeypatch.setattr(ops, "_req", dtype_only)
    lg, te = torch.randn(4, 9), torch.randn(4, 9)
    for bad in (te.double(), te.half(), te.to(torch.bfloat16)):
        with pytest.raises(TypeError, match="teacher"):
            ops.kl_rows(lg, bad)
    for bad in (te[:3], te[:, :8], torch.randn(9, 4).t(), torch.randn(4, 18)[:, ::2], te.to("meta")):
        with pytest.raises(ValueError, match="teacher"):
            ops.kl_rows(lg, bad)
    with pytest.raises(TypeError, match="agree"):
        ops.kl_rows(lg, te, agree=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="loss_row"):
        ops.kl_rows(lg, te, loss_row=torch.zeros(5))
    with pytest.raises(ValueError, match="dlogits"):
        ops.kl_rows(lg, te, dlogits=torch.zeros(4, 8))
    with pytest.raises(ValueError, match="rowdot"):
        ops.kl_rows(lg, te, rowdot=torch.zeros(4))                           # a row sum without dlogits


def test_live_group_is_refused(closs, tmp_path, monkeypatch):
    fi, ft, ti, tt = _inputs(4, 4, 8, 8, 10)
    monkeypatch.setenv("CCLIP_DP_FORCE_COLLECTIVES", "1")                    # a one-rank group counts as live
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match="single-process only"):
            closs.distill_loss(fi, ft, torch.tensor(1.0), ti, tt, 20.0)
        with pytest.raises(NotImplementedError):
            closs.DistillLoss(20.0)(fi, ft, torch.tensor(1.0), ti, tt)
    finally:
        dist.destroy_process_group()
    closs.distill_loss(fi, ft, torch.tensor(1.0), ti, tt, 20.0)              # and without one it runs


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_launcher_is_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cclip_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+cclip_kl_rows\s*\(([^)]*)\)\s*;", code)
    assert m, "cclip_kl_rows is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float* logits", "int64_t ld", "const float* teacher", "int64_t ldt", "int32_t R", "int32_t C",
                    "float grad_scale", "float* loss_row", "int32_t* pred", "float* agree", "float* dlogits", "int64_t ldd",
                    "float* rowdot", "hipStream_t stream"]
    assert re.search(r"#define\s+CCLIP_ABI_VERSION\s+3\b", hdr)              # additive: the ABI version does not move
    import __graft_entry__ as ge
    ge.build()
    from cclip_hip import load_library, ops
    assert hasattr(load_library(), "cclip_kl_rows"), "cclip_kl_rows declared in include/cclip_hip.h but not exported"
    assert callable(ops.kl_rows)


# ---- scripts/train_clip.py -------------------------------------------------------------------------------------------------
def _model(resolution, context_length=77, vocab_size=49408):
    return types.SimpleNamespace(visual=types.SimpleNamespace(input_resolution=resolution), context_length=context_length,
                                 vocab_size=vocab_size)


def test_script_options_and_the_resolution_refusal():
    import train_clip
    ap = train_clip.build_args()
    args = ap.parse_args(["--synthetic"])
    assert args.distill_from is None and args.distill_arch is None and args.distill_weight == 1.0
    args = ap.parse_args(["--synthetic", "--distill-from", "pretrained", "--distill-arch", "ViT-B/16", "--distill-weight", "0.5",
                          "--class-aware", "--loss", "sigmoid"])
    assert (args.distill_from, args.distill_arch, args.distill_weight) == ("pretrained", "ViT-B/16", 0.5)
    assert train_clip.load_teacher(ap.parse_args(["--synthetic"]), _model(224), "cpu") == (None, None)
    train_clip.check_teacher(_model(224), _model(224))
    with pytest.raises(ValueError, match="input resolution"):
        train_clip.check_teacher(_model(224), _model(336))                   # ViT-L/14@336px against a 224 student
    with pytest.raises(ValueError, match="context_length"):
        train_clip.check_teacher(_model(224), _model(224, context_length=32))
    with pytest.raises(ValueError, match="neither"):
        train_clip.load_teacher(ap.parse_args(["--distill-from", "/no/such/checkpoint.pt"]), _model(224), "cpu")
