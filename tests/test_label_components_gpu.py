"""Connected components on the device (csrc/label_components.hip, ops.label_components / ops.component_stats,
clip.label_components) against the host flood fill of label_components_ref.py.  Every output is an integer in a canonical form,
so every comparison is for exact equality; both connectivities run on every map.  The maps (label_components_ref.MAPS) are the
smallest at which each mechanism can go wrong: sides below, at and just past the 32 x 32 tile, widths that are no multiple of the
four pixels a thread owns, components that run through many tiles, and batches whose images must not join."""
from __future__ import annotations

import functools
import json
import os
import subprocess
import sys
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import label_components_ref as LR  # noqa: E402

GUARD = 64
CASES = dict(LR.MAPS, **LR.BATCHES)
STATS = ("label", "image", "first", "area", "boxes")


def _ops():
    from cclip_hip import ops
    return ops


def _guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


@functools.lru_cache(maxsize=None)
def _conf(name):
    return LR.confidences(CASES[name].shape, seed=sorted(CASES).index(name))


@functools.lru_cache(maxsize=None)
def _ref(name, connectivity):
    return LR.components(CASES[name], _conf(name), connectivity)


def _device(labels_np, connectivity, conf_np=None):
    """the two native calls on guarded buffers (the guards checked) -> what the reference returns, as numpy arrays"""
    ops = _ops()
    lab = torch.from_numpy(np.ascontiguousarray(labels_np)).cuda()
    lab = lab.reshape((-1,) + tuple(lab.shape[-2:]))
    shape = tuple(lab.shape)
    groups = (lab.numel() + ops.COMPONENTS_GROUP - 1) // ops.COMPONENTS_GROUP
    rbuf, root = _guarded(shape, torch.int32, -77)
    ibuf, ids = _guarded(shape, torch.int32, -77)
    cbuf, count = _guarded((1,), torch.int32, -77)
    wbuf, ws = _guarded((groups,), torch.int32, -77)
    ops.label_components(lab, connectivity, root, ids, count, ws)
    n = int(count.item())
    assert _intact(rbuf, -77) and _intact(ibuf, -77) and _intact(cbuf, -77) and _intact(wbuf, -77)
    conf = None if conf_np is None else torch.from_numpy(conf_np).cuda().reshape(shape)
    bufs = dict(label=_guarded((n,), torch.uint8, 77), image=_guarded((n,), torch.int32, -77), first=_guarded((n,), torch.int32, -77),
                area=_guarded((n,), torch.int32, -77), boxes=_guarded((n, 4), torch.int32, -77))
    qbuf, qsum = _guarded((n,), torch.int64, -77) if conf is not None else (None, None)
    ops.component_stats(lab, root, ids, n, bufs["label"][1], bufs["image"][1], bufs["first"][1], bufs["area"][1], bufs["boxes"][1],
                        conf=conf, qsum=qsum)
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _intact(buf, 77 if k == "label" else -77), k
    assert qbuf is None or _intact(qbuf, -77)
    assert _intact(rbuf, -77) and _intact(ibuf, -77)
    out = dict(root=root.cpu().numpy().reshape(labels_np.shape), ids=ids.cpu().numpy().reshape(labels_np.shape), n=n,
               qsum=None if qsum is None else qsum.cpu().numpy().astype(np.uint64))
    out.update({k: v.cpu().numpy() for k, (_, v) in bufs.items()})
    return out


def _same(got, ref, tag):
    assert got["n"] == ref["n"], f"{tag}: count {got['n']} != {ref['n']}"
    for k in ("root", "ids") + STATS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, f"{tag}: {k} {got[k].dtype} {got[k].shape}"
        bad = np.flatnonzero((got[k] != ref[k]).reshape(-1))
        assert bad.size == 0, f"{tag}: {k} differs at {bad.size} places, first flat index {bad[0]}: {got[k].reshape(-1)[bad[0]]} != {ref[k].reshape(-1)[bad[0]]}"
    if ref["qsum"] is not None and got["qsum"] is not None:
        assert np.array_equal(got["qsum"], ref["qsum"]), f"{tag}: qsum"


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(CASES))
def test_components_equal_the_flood_fill(name, connectivity):
    ref = _ref(name, connectivity)
    got = _device(CASES[name], connectivity, _conf(name))
    _same(got, ref, f"{name} / {connectivity}")
    assert got["qsum"] is not None and got["qsum"].dtype == np.uint64


def test_known_answers_on_the_device():
    one = _device(LR.MAPS["one_class_97x130"], 4)
    assert one["n"] == 1 and one["area"].tolist() == [97 * 130] and one["boxes"].tolist() == [[0, 0, 130, 97]] and one["qsum"] is None
    assert _device(LR.MAPS["checkerboard_66x70"], 4)["n"] == 66 * 70
    assert _device(LR.MAPS["checkerboard_66x70"], 8)["n"] == 2
    arms = _device(LR.MAPS["arms_70x70"], 4)
    assert arms["n"] == 1 and arms["first"].tolist() == [3 * 70 + 60]
    none = _device(np.full((5, 37), LR.NONE, dtype=np.uint8), 8)
    assert none["n"] == 0 and (none["root"] == -1).all() and (none["ids"] == -1).all()


def test_qsum_on_the_edges_of_the_fixed_point():
    """one component that holds every planted value (0, 1, 0.5 - 2^-25, 1 + 1e-3, a negative, NaN, inf, 2^-17, 1 - 2^-24), and one
    pixel per component so that every q() is seen on its own"""
    conf = LR.confidences((33, 65), seed=50)
    whole = np.zeros((33, 65), dtype=np.uint8)
    got, ref = _device(whole, 4, conf), LR.components(whole, conf, 4)
    assert got["qsum"].tolist() == ref["qsum"].tolist() == [int(LR.quantise(conf).sum())]
    cb = LR.checkerboard(33, 65)
    got, ref = _device(cb, 4, conf), LR.components(cb, conf, 4)
    assert got["n"] == 33 * 65 and np.array_equal(got["qsum"], LR.quantise(conf).reshape(-1)) and np.array_equal(got["qsum"], ref["qsum"])


def test_two_calls_give_equal_bytes():
    name = "percolation_130x257"
    for connectivity in (4, 8):
        a, b = _device(CASES[name], connectivity, _conf(name)), _device(CASES[name], connectivity, _conf(name))
        for k in ("root", "ids", "qsum") + STATS:
            assert a[k].tobytes() == b[k].tobytes(), (k, connectivity)
        assert a["n"] == b["n"]


@pytest.mark.parametrize("name", LR.RANDOM_MAPS)
def test_boxes_of_is_label_boxes(name):
    import clip
    m = LR.MAPS[name]
    labels = torch.from_numpy(m).cuda()
    res = clip.label_components(labels, torch.from_numpy(_conf(name)).cuda())
    ref = _ref(name, 4)
    assert res.n == ref["n"] and res.ids.shape == labels.shape and res.root.dtype == torch.int32 and res.connectivity == 4
    assert np.array_equal(res.ids.cpu().numpy(), ref["ids"]) and np.array_equal(res.root.cpu().numpy(), ref["root"])
    assert not res.boxes.is_cuda and res.score.dtype == torch.float64
    assert np.array_equal(res.score.numpy(), ref["qsum"].astype(np.float64) / (65536.0 * ref["area"].astype(np.float64)))
    for c in sorted(set(np.unique(m).tolist()) - {LR.NONE}) + [7]:
        for min_area in (1, 5):
            assert res.boxes_of(c, min_area) == clip.label_boxes(labels, c, min_area), (name, c, min_area)
    i = int(np.argmax(ref["area"]))
    assert np.array_equal(res.mask(i).cpu().numpy(), ref["ids"] == i)
    assert res.instances(min_area=5, min_score=0.4, classes=[0], class_names=["a", "b", "c"]) == \
        [r for r in LR.instances(ref, ["a", "b", "c"], min_area=5, min_score=0.4) if r["class"] == 0]


def test_batch_through_the_public_call():
    import clip
    name = "different_3x33x65"
    b = LR.BATCHES[name]
    res = clip.label_components(torch.from_numpy(b).cuda(), connectivity=8)
    ref = _ref(name, 8)
    assert res.score is None and res.n == ref["n"] and np.array_equal(res.image.numpy(), ref["image"])
    assert np.array_equal(res.boxes.numpy(), ref["boxes"]) and np.array_equal(res.area.numpy(), ref["area"])
    for i in range(3):
        assert res.boxes_of(1, 2, image=i) == LR.boxes_of(ref, 1, 2, image=i)
    assert res.instances() == LR.instances(dict(ref, qsum=None))


# ---- argument errors ---------------------------------------------------------------------------
def test_raw_library_argument_errors():
    from cclip_hip import load_library
    lib = load_library()
    z = c_void_p(0)
    ERR_ARG = lib.cclip_label_components(z, c_int(1), c_int(1), c_int(1), c_int(4), z, z, z, z, c_int64(1), z)
    assert ERR_ARG == 1
    lab = torch.zeros(2, 5, 7, device="cuda", dtype=torch.uint8)
    root = torch.full((2 * 5 * 7 + 1,), -77, device="cuda", dtype=torch.int32)
    ids, count, ws = torch.full_like(root, -77), torch.full((1,), -77, device="cuda", dtype=torch.int32), torch.zeros(4, device="cuda", dtype=torch.int32)
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(labels=lab.data_ptr(), B=2, H=5, W=7, conn=4, root=root.data_ptr(), ids=ids.data_ptr(), count=count.data_ptr(),
                ws=ws.data_ptr(), ws_ints=4)

    def call(**kw):
        a = dict(good, **kw)
        return lib.cclip_label_components(c_void_p(a["labels"]), c_int(a["B"]), c_int(a["H"]), c_int(a["W"]), c_int(a["conn"]), c_void_p(a["root"]),
                                          c_void_p(a["ids"]), c_void_p(a["count"]), c_void_p(a["ws"]), c_int64(a["ws_ints"]), stream)

    bad = [dict(labels=0), dict(root=0), dict(ids=0), dict(count=0), dict(ws=0), dict(conn=6), dict(conn=0), dict(B=0), dict(H=0), dict(W=0),
           dict(H=16385), dict(W=16385), dict(B=8, H=16384, W=16384), dict(B=1 << 30, H=2, W=1), dict(root=root.data_ptr() + 2),
           dict(ids=ids.data_ptr() + 1), dict(count=count.data_ptr() + 2), dict(ws=ws.data_ptr() + 2), dict(ws_ints=0)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (root == -77).all() and (ids == -77).all() and (count == -77).all()           # nothing was launched
    assert call(labels=lab.data_ptr() + 1, B=1) == 0                                       # labels may have any alignment
    torch.cuda.synchronize()
    assert int(count.item()) == 1

    assert call() == 0
    n = 1
    label = torch.zeros(n, device="cuda", dtype=torch.uint8)
    image, first, area = (torch.full((n + 1,), -77, device="cuda", dtype=torch.int32) for _ in range(3))
    box = torch.full((4 * n + 1,), -77, device="cuda", dtype=torch.int32)
    qsum = torch.full((n + 1,), -77, device="cuda", dtype=torch.int64)
    conf = torch.rand(2 * 5 * 7 + 1, device="cuda")
    sgood = dict(labels=lab.data_ptr(), conf=conf.data_ptr(), root=root.data_ptr(), ids=ids.data_ptr(), B=2, H=5, W=7, n=n, label=label.data_ptr(),
                 image=image.data_ptr(), first=first.data_ptr(), area=area.data_ptr(), box=box.data_ptr(), qsum=qsum.data_ptr())

    def stats(**kw):
        a = dict(sgood, **kw)
        return lib.cclip_component_stats(c_void_p(a["labels"]), c_void_p(a["conf"]), c_void_p(a["root"]), c_void_p(a["ids"]), c_int(a["B"]),
                                         c_int(a["H"]), c_int(a["W"]), c_int(a["n"]), c_void_p(a["label"]), c_void_p(a["image"]), c_void_p(a["first"]),
                                         c_void_p(a["area"]), c_void_p(a["box"]), c_void_p(a["qsum"]), stream)

    sbad = [dict(labels=0), dict(root=0), dict(ids=0), dict(label=0), dict(image=0), dict(first=0), dict(area=0), dict(box=0), dict(conf=0),
            dict(qsum=0), dict(n=-1), dict(n=71), dict(H=0), dict(W=16385), dict(B=8, H=16384, W=16384), dict(root=root.data_ptr() + 2),
            dict(conf=conf.data_ptr() + 2), dict(area=area.data_ptr() + 2), dict(box=box.data_ptr() + 1), dict(qsum=qsum.data_ptr() + 4)]
    for kw in sbad:
        assert stats(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (area == -77).all() and (box == -77).all() and (qsum == -77).all()
    assert stats(n=0, label=0, image=0, first=0, area=0, box=0) == 0                       # nothing to describe: nothing launched
    assert stats() == 0 and stats(conf=0, qsum=0) == 0
    torch.cuda.synchronize()
    assert area[:1].tolist() == [35] and box[:4].tolist() == [0, 0, 7, 5] and image[:1].tolist() == [0]   # n = 1 of the 2: id 1 is passed over


def test_wrapper_argument_errors():
    import clip
    ops = _ops()
    lab = torch.zeros(2, 5, 7, device="cuda", dtype=torch.uint8)
    root, ids = torch.empty(2, 5, 7, device="cuda", dtype=torch.int32), torch.empty(2, 5, 7, device="cuda", dtype=torch.int32)
    count, ws = torch.empty(1, device="cuda", dtype=torch.int32), torch.empty(1, device="cuda", dtype=torch.int32)
    ops.label_components(lab, 4, root, ids, count, ws)
    lc = ops.label_components
    cases = [
        ("label_components: labels must be a cuda tensor", lambda: lc(lab.cpu(), 4, root, ids, count, ws)),
        ("label_components: labels must be torch.uint8", lambda: lc(lab.int(), 4, root, ids, count, ws)),
        ("label_components: labels must be contiguous", lambda: lc(lab.transpose(1, 2), 4, root, ids, count, ws)),
        ("label_components: labels must be \\[B, H, W\\]", lambda: lc(lab[0], 4, root, ids, count, ws)),
        ("label_components: root must be a cuda tensor", lambda: lc(lab, 4, root.cpu(), ids, count, ws)),
        ("label_components: root must be torch.int32", lambda: lc(lab, 4, root.long(), ids, count, ws)),
        ("label_components: ids must be \\[2, 5, 7\\]", lambda: lc(lab, 4, root, ids.view(2, 7, 5), count, ws)),
        ("label_components: count must be torch.int32", lambda: lc(lab, 4, root, ids, count.long(), ws)),
        ("label_components: count must hold one element", lambda: lc(lab, 4, root, ids, ws.new_empty(2), ws)),
        ("label_components: workspace must be a cuda tensor", lambda: lc(lab, 4, root, ids, count, ws.cpu())),
        ("label_components: workspace must hold at least 1", lambda: lc(lab, 4, root, ids, count, ws[:0])),
        ("label_components: connectivity must be 4 or 8, got 6", lambda: lc(lab, 6, root, ids, count, ws)),
        ("label_components: height 1, width 16385", lambda: lc(torch.zeros(1, 1, 16385, device="cuda", dtype=torch.uint8), 4, root, ids, count, ws)),
    ]
    n = int(count.item())
    assert n == 2
    label = torch.empty(n, device="cuda", dtype=torch.uint8)
    image, first, area = (torch.empty(n, device="cuda", dtype=torch.int32) for _ in range(3))
    box, qsum, conf = torch.empty(n, 4, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.int64), torch.rand(2, 5, 7, device="cuda")
    cs = ops.component_stats
    cs(lab, root, ids, n, label, image, first, area, box, conf=conf, qsum=qsum)
    assert area.tolist() == [35, 35] and image.tolist() == [0, 1] and first.tolist() == [0, 35]
    cases += [
        ("component_stats: labels must be a cuda tensor", lambda: cs(lab.cpu(), root, ids, n, label, image, first, area, box)),
        ("component_stats: ids must be torch.int32", lambda: cs(lab, root, ids.long(), n, label, image, first, area, box)),
        ("component_stats: conf must be torch.float32", lambda: cs(lab, root, ids, n, label, image, first, area, box, conf=conf.double(), qsum=qsum)),
        ("component_stats: conf must be \\[2, 5, 7\\]", lambda: cs(lab, root, ids, n, label, image, first, area, box, conf=conf[0], qsum=qsum)),
        ("component_stats: label must be torch.uint8", lambda: cs(lab, root, ids, n, area, image, first, area, box)),
        ("component_stats: qsum must be torch.int64", lambda: cs(lab, root, ids, n, label, image, first, area, box, conf=conf, qsum=area)),
        ("component_stats: conf and qsum go together", lambda: cs(lab, root, ids, n, label, image, first, area, box, conf=conf)),
        ("component_stats: n must be an integer in \\[0, 70\\]", lambda: cs(lab, root, ids, 71, label, image, first, area, box)),
        ("component_stats: box must be \\[2, 4\\]", lambda: cs(lab, root, ids, n, label, image, first, area, box.view(4, 2))),
        ("component_stats: area must be \\[2\\]", lambda: cs(lab, root, ids, n, label, image, first, area[:1], box)),
        ("label_components: labels must be \\[H, W\\] or \\[B, H, W\\]", lambda: clip.label_components(lab[0, 0])),
        ("label_components: conf must be a tensor of the labels' shape", lambda: clip.label_components(lab, conf[0])),
        ("label_components: connectivity must be 4 or 8", lambda: clip.label_components(lab, connectivity=5)),
    ]
    for match, fn in cases:
        with pytest.raises(ValueError, match=match):
            fn()


# ---- end to end: the toy towers of test_dense_stitch_gpu.py ------------------------------------------
def _toy(grid, dtype, seed=11):
    import clip
    from clip.weights import CLIPGeometry, init_state_dict
    geo = CLIPGeometry(64, 32 * grid, 2, 128, 32, 16, 512, 128, 2, 2)       # width 128, 2 heads of 64, 2 layers
    sd = init_state_dict(geo, seed)
    return geo, sd, clip.build_model(sd, dtype).cuda().eval()


def test_segment_photo_instances():
    import clip
    geo, sd, model = _toy(2, torch.bfloat16)
    photo = torch.randint(0, 256, (45, 61, 3), generator=torch.Generator().manual_seed(21), dtype=torch.uint8)
    text = torch.randn(4, geo.embed_dim, generator=torch.Generator().manual_seed(2)).cuda()
    res = clip.segment_photo(model, photo, text, window=24, stride=12, min_conf=0.3, batch=4)
    for connectivity in (4, 8):
        ref = LR.components(res.labels.cpu().numpy(), res.conf.cpu().numpy(), connectivity)
        assert ref["n"] >= 2
        assert res.instances(connectivity=connectivity) == LR.instances(ref)
        assert res.instances(min_area=4, min_score=0.3, connectivity=connectivity) == LR.instances(ref, min_area=4, min_score=0.3)
        comps = res.components(connectivity)
        assert np.array_equal(comps.ids.cpu().numpy(), ref["ids"]) and np.array_equal(comps.qsum.numpy().astype(np.uint64), ref["qsum"])
    for c in range(4):
        assert res.components().boxes_of(c, 3) == res.class_boxes(c, 3)
    dense = clip.segment(model, torch.randn(2, 3, geo.image_resolution, geo.image_resolution, generator=torch.Generator().manual_seed(5)).cuda(),
                         text, size=(37, 50))
    ref = LR.components(dense.labels.cpu().numpy(), dense.conf.cpu().numpy(), 4)
    assert dense.instances() == LR.instances(ref) and {r["image"] for r in dense.instances()} == {0, 1}


def test_segment_images_script_with_instances(tmp_path):
    """the records the script prints are the reference's on the label map the same pipeline gives in this process"""
    import clip
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import _common as C
    import segment_images as SI
    from PIL import Image
    argv = ["--synthetic", "--n_images", "2", "--size", "40", "--instances", "--min-area", "3", "--connectivity", "8"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "segment_images.py"), *argv], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and all("instances" in l for l in lines)

    args = SI.build_parser().parse_args(argv)
    C.make_synthetic_annotations(str(tmp_path), per_class=1 + (args.n_images - 1) // len(C.CLASSES))
    d = os.path.join(str(tmp_path), "images")
    files = [os.path.join(d, f) for f in sorted(os.listdir(d))][:args.n_images]
    assert [os.path.basename(f) for f in files] == [os.path.basename(l["file"]) for l in lines]
    model, preprocess = clip.load("test-tiny", device=torch.device("cuda:0"), jit=False)
    model.eval()
    prompts = SI.class_prompts(args)
    with torch.no_grad():
        text = model.encode_text(C.get_tokenize(model)(prompts).to("cuda:0")).float()
    image = torch.stack([preprocess(Image.open(f).convert("RGB")) for f in files]).to("cuda:0")
    res = clip.segment(model, image, text, size=40)
    ref = LR.components(res.labels.cpu().numpy(), res.conf.cpu().numpy(), 8)
    for j, line in enumerate(lines):
        want = [{"class": r["class"], "name": r["name"], "box": list(r["box"]), "area": r["area"], "score": round(r["score"], 6)}
                for r in LR.instances(ref, prompts, min_area=3) if r["image"] == j]
        assert line["instances"] == want and len(want) >= 1
