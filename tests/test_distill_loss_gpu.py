"""GPU: clip.distill_loss / clip.DistillLoss on the built library, and scripts/train_clip.py --distill-from, against the float64
evaluation of the definition (distill_loss_helpers.ref_loss: kl_div over log_softmax of the scaled cosines, both directions,
gradients by autograd).

Bounds: absolute, H.LOSS_TOL_GPU = 4 x the largest deviation of the value and of each of the three gradients measured on an
MI355X over the three cases below.  Every case prints its figures before it asserts."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "scripts")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import distill_loss_helpers as H  # noqa: E402

LS, TS = 2.6593, 50.0              # the student's log(1 / 0.07); a teacher whose scale has grown to 50


def _features(N, M, E, Et, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(N, E, device="cuda", generator=gen, requires_grad=True),
            torch.randn(M, E, device="cuda", generator=gen, requires_grad=True),
            torch.randn(N, Et, device="cuda", generator=gen), torch.randn(M, Et, device="cuda", generator=gen))


# square, rectangular (the distinct texts of a batch), a teacher of another embedding width
@pytest.mark.parametrize("N,M,E,Et", [(16, 16, 64, 64), (16, 5, 64, 64), (16, 16, 64, 96)])
def test_loss_against_float64(N, M, E, Et):
    import clip
    fi, ft, ti, tt = _features(N, M, E, Et, N * 100 + M + Et)
    ls = torch.tensor(LS, device="cuda", requires_grad=True)
    loss, stats = clip.distill_loss(fi, ft, ls, ti, tt, TS)
    loss.backward()
    torch.cuda.synchronize()
    ref, agree, dfi, dft, dls, _ = H.ref_loss_and_grads(fi, ft, ls, ti, tt, TS)
    dev = (abs(loss.item() - ref.item()), (fi.grad.double() - dfi).abs().max().item(), (ft.grad.double() - dft).abs().max().item(),
           abs(ls.grad.item() - dls.item()))
    print(f"distill_loss dev [{N},{M}] E={E} Et={Et}: loss {dev[0]:.3e} dfi {dev[1]:.3e} dft {dev[2]:.3e} dls {dev[3]:.3e}"
          f" | loss {loss.item():.6f} max |dfi| {dfi.abs().max().item():.3e} max |dft| {dft.abs().max().item():.3e} dls {dls.item():.3e}"
          f" | agree {int(stats[1].item())} ref {agree}")
    assert all(v <= t for v, t in zip(dev, H.LOSS_TOL_GPU)), dev
    assert stats.shape == (2,) and not stats.requires_grad and stats[0].item() == loss.item()
    assert int(stats[1].item()) == agree
    assert ti.grad is None and tt.grad is None and ls.grad.shape == ()


def test_teacher_equal_to_student_and_the_module():
    import clip
    fi, ft, _, _ = _features(16, 5, 64, 64, 7)
    ls = torch.tensor(LS, device="cuda", requires_grad=True)
    mod = clip.DistillLoss(ls.detach().exp()).to("cuda")
    assert list(mod.parameters()) == [] and mod.teacher_scale.is_cuda
    loss, stats = mod(fi, ft, ls, fi.detach().clone(), ft.detach().clone())
    loss.backward()
    print(f"teacher == student: loss {loss.item():.3e} max |dfi| {fi.grad.abs().max().item():.3e} dls {ls.grad.item():.3e}")
    # the teacher's scale passes through log and exp: its logits differ from the student's by that rounding alone, and the
    # deviation bounds of the general case cover a value that is 0 in float64
    assert 0.0 <= loss.item() <= H.LOSS_TOL_GPU[0] and int(stats[1].item()) == 16
    assert fi.grad.abs().max().item() <= H.LOSS_TOL_GPU[1] and ft.grad.abs().max().item() <= H.LOSS_TOL_GPU[2]
    assert abs(ls.grad.item()) <= H.LOSS_TOL_GPU[3]


def test_refusals_on_the_device():
    import clip
    fi, ft, ti, tt = _features(16, 5, 64, 96, 8)
    ls = torch.tensor(LS, device="cuda")
    with pytest.raises(ValueError, match="teacher_image_features"):
        clip.distill_loss(fi, ft, ls, ti[:15], tt, TS)
    with pytest.raises(ValueError, match="teacher_text_features"):
        clip.distill_loss(fi, ft, ls, ti, tt[:4], TS)


def test_one_step_leaves_the_teacher_model_alone():
    import clip
    from clip import optim as coptim
    from clip.weights import MODELS, init_state_dict, synthetic_images, synthetic_text
    geo = MODELS["test-small"]
    model = clip.build_model(init_state_dict(geo, 3)).to("cuda:0")
    teacher = clip.build_model(init_state_dict(geo, 4)).to("cuda:0")
    model.train()
    teacher.eval()
    teacher.requires_grad_(False)
    slots = teacher.arena.gflat
    slots.fill_(0.25)
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    mine = {k: v.clone() for k, v in model.state_dict().items()}
    img, txt = synthetic_images(6, geo, 4).cuda(), synthetic_text(6, geo, 5).cuda()
    opt = coptim.AdamW(model, lr=1e-4)
    distill = clip.DistillLoss(teacher.logit_scale.detach().exp()).to("cuda")
    fi, ft = model.encode_image_text(img, txt)
    with torch.no_grad():
        tfi, tft = teacher.encode_image_text(img, txt)
    hard, _ = clip.contrastive_loss(fi, ft, model.logit_scale, None)
    soft, stats = distill(fi, ft, model.logit_scale, tfi, tft)
    (hard + 0.5 * soft).backward()
    opt.step()
    torch.cuda.synchronize()
    print(f"hard {hard.item():.5f} distill {soft.item():.5f} agree {int(stats[1].item())} of 6")
    assert torch.isfinite(hard) and torch.isfinite(soft) and soft.item() > 0.0
    after = teacher.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert torch.equal(slots, torch.full_like(slots, 0.25)) and all(p.grad is None for p in teacher.parameters())
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, mine[k])]
    assert moved and "logit_scale" in moved                                  # the student did take the step


def test_train_clip_script_distils(tmp_path, capsys, monkeypatch):
    import train_clip
    monkeypatch.setenv("CCLIP_COMPUTE_DTYPE", "bf16")
    n = train_clip.main(["--synthetic", "--model", "test-small", "--distill-from", "pretrained", "--distill-weight", "0.5",
                         "--class-aware", "--max-steps", "2", "--batch-size", "2", "--epochs", "1", "--out-dir", str(tmp_path),
                         "--warmup-steps", "0", "--lr", "1e-4"])
    assert n == 2
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "loss" in l]
    assert len(steps) == 2
    for l in steps:
        print(l)
        for key in ("loss", "hard", "distill"):
            assert torch.isfinite(torch.tensor(l[key]))
        assert l["distill"] >= 0.0 and 0.0 <= l["agree"] <= 1.0 and 0.0 <= l["accuracy"] <= 1.0
        assert abs(l["loss"] - (l["hard"] + 0.5 * l["distill"])) <= 1e-4
