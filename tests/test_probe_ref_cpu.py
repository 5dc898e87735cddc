"""CPU: the float64 linear-probe reference (tests/probe_ref.py) against torch.autograd, its tolerances against planted faults,
and the host-side pieces of clip/probe.py and scripts/linear_probe.py.  No kernel runs here."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

import probe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

DTYPES = [torch.bfloat16, torch.float16]


def problem(dtype, N=300, C=5, D=64, seed=3, exact_w=False):
    gen = torch.Generator().manual_seed(seed)
    x16 = torch.randn(N, D, generator=gen).to(dtype)
    W = torch.randn(C, D, generator=gen) * 0.7
    if exact_w:
        W = W.to(dtype).float()                                             # lo == 0: hi + lo is W itself
    b = torch.randn(C, generator=gen)
    y = torch.randint(0, C, (N,), generator=gen)
    y[::17] = -1
    y[5] = C + 3
    rw = torch.rand(N, generator=gen)
    rw[7], rw[9], rw[11] = 0.0, float("nan"), 3.0
    return x16, W, b, y, rw


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_reference_equals_autograd_cross_entropy(dtype):
    x16, W, b, y, _ = problem(dtype, exact_w=True)
    C = W.shape[0]
    cw = torch.tensor([1.0, 0.5, 0.25, 1.0, 0.125], dtype=torch.float64)          # exact in fp32, as the kernel's weights are
    yc = torch.where((y >= 0) & (y < C), y, torch.full_like(y, -100))
    rw = torch.where(yc >= 0, cw[yc.clamp(min=0)], torch.zeros(1, dtype=torch.float64)).float()
    scale, l2 = 1.0 / float(rw.sum()), 0.03
    ref = R.reference(x16, W, b, y, rw, scale, l2)
    Wp, bp = W.double().requires_grad_(True), b.double().requires_grad_(True)
    # weighted mean reduction of F.cross_entropy divides by the sum of the weights of the live rows: scale above
    f = F.cross_entropy(x16.double() @ Wp.t() + bp, yc, weight=cw, ignore_index=-100) + 0.5 * l2 * (Wp * Wp).sum()
    f.backward()
    assert abs(ref["objective"].item() - f.item()) < 1e-12 * max(1.0, abs(f.item()))
    assert (ref["dW"] - Wp.grad).abs().max().item() < 1e-12
    assert (ref["db"] - bp.grad).abs().max().item() < 1e-12
    assert torch.equal(ref["pred"], (x16.double() @ W.double().t() + b.double()).argmax(dim=1))
    # and the stand-alone objective function agrees with the dict
    f2 = R.objective64(x16, W.double(), b.double(), y, rw, scale, l2)
    assert abs(f2.item() - f.item()) < 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_split_and_selection(dtype):
    x16, W, b, y, rw = problem(dtype)
    hi, lo = R.split16(W, dtype)
    rem = (W.double() - hi.double() - lo.double()).abs().max().item()
    assert 0 < (lo.double().abs().max().item()) and rem <= R.SPLIT[dtype][0] * W.abs().max().item() + R.SPLIT[dtype][1]
    x = x16.clone()
    x[0] = float("nan"); y[0] = -1                                          # an ignored NaN row
    x[7] = float("nan")                                                     # a zero-weight NaN row
    ref = R.reference(x, W, b, y, rw, 0.01, 0.1)
    assert ref["loss"][0].item() == 0 and ref["loss"][7].item() == 0 and ref["loss"][9].item() == 0
    assert torch.isfinite(ref["dW"]).all() and torch.isfinite(ref["db"]).all() and torch.isfinite(ref["objective"])
    assert torch.isfinite(ref["dW_tol"]).all() and torch.isfinite(ref["obj_tol"])
    assert not ref["live"][5] and not ref["live"][9]                        # label >= C; NaN weight
    w11 = R.clamp_weights(rw, x.shape[0])[11].item()
    assert w11 == 1.0                                                       # 3.0 clamps to 1


def test_argmax_order():
    nan = float("nan")
    z = torch.tensor([[1.0, 2.0, 2.0], [nan, -5.0, nan], [nan, nan, nan], [0.0, -0.0, -1.0], [-float("inf"), nan, -float("inf")]],
                     dtype=torch.float64)
    assert R.argmax_ref(z).tolist() == [1, 1, 0, 0, 0]


FAULTS = ["drop_lo", "bias_not_in_lse", "onehot_wrong_class", "ignored_row_leaks", "missing_part", "l2_on_bias"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fault", FAULTS)
def test_tolerance_sees_planted_fault(fault, dtype):
    """A kernel with the fault would differ from the reference by more than the derived bound in some output."""
    x16, W, b, y, rw = problem(dtype, N=700)
    scale, l2 = 1.0 / 600, 0.05
    ref = R.reference(x16, W, b, y, rw, scale, l2)
    bad = R.reference(x16, W, b, y, rw, scale, l2, fault=fault)
    seen = []
    for k in ("z", "lse", "loss", "dW", "db"):
        tol = ref[{"z": "z_tol", "lse": "lse_tol", "loss": "loss_tol", "dW": "dW_tol", "db": "db_tol"}[k]]
        ok = torch.isfinite(tol) & torch.isfinite(ref[k])
        if ((bad[k] - ref[k]).abs()[ok] > tol[ok]).any():
            seen.append(k)
    if abs(bad["objective"].item() - ref["objective"].item()) > ref["obj_tol"].item():
        seen.append("objective")
    expect = {"drop_lo": "z", "bias_not_in_lse": "lse", "onehot_wrong_class": "dW", "ignored_row_leaks": "loss",
              "missing_part": "dW", "l2_on_bias": "db"}[fault]
    assert expect in seen, (fault, seen)
    # the bounds are tight enough to be useful: far below the quantities they guard
    assert ref["dW_tol"].max().item() < 1e-2 * ref["dW"].abs().max().item()
    assert ref["obj_tol"].item() < 1e-4 * ref["objective"].item()


def test_geometry_closed_form():
    assert R.geometry(256, 5, 64) == (4, 8, 4) and R.geometry(257, 5, 64)[2] == 8           # P goes from 1 to 2 at N = 257
    assert R.geometry(256, 64, 64)[2] == 1 and R.geometry(257, 64, 64)[2] == 2
    rs, tpp, S = R.geometry(10 ** 6, 256, 512)
    assert rs == 1 and S * 256 * 512 * 4 <= 1 << 25 and S == -(-31250 // tpp)
    assert R.workspace_bytes(3000, 16, 512) == 4 * 16 * 512 + 4 * R.geometry(3000, 16, 512)[2] * 16 * 513 + 4 * (32 + 256)


# ---- host logic of clip/probe.py --------------------------------------------------------------------------------------
def test_balanced_weights_and_scale():
    from clip.probe import probe_weights
    y = torch.tensor([0] * 20 + [1] * 2 + [-1] * 3 + [7])                   # 10 : 1, three ignored, one label >= C
    rw, scale = probe_weights(y, 2, "balanced")
    L = 22
    raw = torch.tensor([L / (2 * 20)] * 20 + [L / (2 * 2)] * 2 + [0.0] * 4)
    assert torch.allclose(rw.double(), (raw / raw.max()).double(), atol=1e-7) and rw.dtype == torch.float32
    assert rw.max().item() == 1.0 and (rw[22:] == 0).all()
    assert abs(scale - raw.max().item() / L) < 1e-15                        # every class present: sum r = L
    # the weighted objective is the weighted mean of the loss
    loss = torch.rand(26, dtype=torch.float64)
    assert abs(scale * (rw.double() * loss).sum().item() - (raw.double() * loss).sum().item() / L) < 1e-7
    none, s1 = probe_weights(y, 2, None)
    assert none is None and s1 == 1.0 / L
    rw3, s3 = probe_weights(y, 2, torch.tensor([2.0, 0.5]))
    assert rw3[:20].eq(1.0).all() and torch.allclose(rw3[20:22], torch.tensor([0.25, 0.25])) and abs(s3 - 2.0 / 41.0) < 1e-15
    with pytest.raises(ValueError):
        probe_weights(y, 2, "bogus")
    with pytest.raises(ValueError):
        probe_weights(y, 2, torch.tensor([1.0, -1.0]))
    assert probe_weights(torch.tensor([-1, -1]), 2, None)[1] == 0.0


def test_sweep_bookkeeping_and_label_mapping():
    from clip.probe import best_row
    from clip.fewshot import _labels_from_metadata
    table = [dict(l2=1.0, val_accuracy=0.5), dict(l2=0.1, val_accuracy=0.8), dict(l2=0.01, val_accuracy=0.8)]
    assert best_row(table) == 1                                             # the first of equals
    with pytest.raises(ValueError):
        best_row([])
    meta = [dict(v="b"), dict(v="a"), dict(v="b")]
    y, names = _labels_from_metadata(meta, "v", None)
    assert y.tolist() == [0, 1, 0] and names == ["b", "a"]


def test_state_dict_round_trip_on_cpu():
    from clip.probe import LinearProbe
    p = LinearProbe(64, class_names=["a", "b", "c"], dtype=torch.float16)
    p.W = torch.randn(3, 64)
    p.bias = torch.randn(3)
    p.l2 = 0.25
    sd = p.state_dict()
    q = LinearProbe.from_state_dict(sd)
    assert torch.equal(q.W, p.W) and torch.equal(q.bias, p.bias) and q.class_names == ["a", "b", "c"] and q.l2 == 0.25
    assert q.dtype == torch.float16 and q.num_classes == 3 and q.dim == 64
    with pytest.raises(KeyError):
        LinearProbe.from_state_dict({k: v for k, v in sd.items() if k != "bias"})
    with pytest.raises(NotImplementedError):
        LinearProbe(48, 3)
    with pytest.raises(NotImplementedError):
        LinearProbe(64, 1)
    with pytest.raises(TypeError):
        p.predict(torch.randn(4, 64))                                       # a CPU tensor: no eager fallback


def test_script_argument_parsing():
    import linear_probe as S
    a = S.parse_args(["emb.pkl", "--key", "violation_type", "--val-fraction", "0.2", "--l2", "1e-3,1e-2", "--class-weight", "balanced"])
    assert a.embeddings == "emb.pkl" and a.l2 == [1e-3, 1e-2] and a.class_weight == "balanced" and a.val is None
    assert a.dedup_threshold is None and a.val_fraction == 0.2
    with pytest.raises(SystemExit):
        S.parse_args(["emb.pkl", "--val", "v.pkl", "--val-fraction", "0.2"])
    with pytest.raises(SystemExit):
        S.parse_args(["emb.pkl", "--class-weight", "other"])
