"""Region preprocess on the device (csrc/preprocess_rois.hip, clip.DevicePreprocess.regions / many, clip.encode_regions /
classify_regions) against the host pipeline `clip._transform(n)(image.crop(box))`.  Every comparison is exact: torch.equal /
np.array_equal, no tolerance anywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

PAIRS = [(640, 298), (61, 224), (224, 224), (1080, 224), (7000, 224), (2, 224)]      # (input size, resized size) of one axis


def _photo(w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    return Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB")


@pytest.fixture(scope="module")
def photo_vga():
    return _photo(640, 480, 11)


@pytest.fixture(scope="module")
def photo_big():
    return _photo(3000, 2000, 12)


def _host(image, boxes, n):
    import clip
    t = clip._transform(n)
    return torch.stack([t(image.crop(tuple(int(v) for v in b))) for b in boxes])


def _vga_boxes(n):
    return [(0, 0, 640, 480), (0, 0, 2, 2), (3, 5, 20, 28), (1, 1, 1 + n, 1 + n), (0, 0, n, 300), (100, 0, 640, 480),
            (639 - 17, 479 - 9, 640, 480), (7, 11, 310, 211)]


def _tables(desc_np, n, ksize_max):
    from cclip_hip import ops
    K = desc_np.shape[0]
    desc_host = torch.from_numpy(desc_np)
    bounds = torch.zeros(K, 2, n, 2, device="cuda", dtype=torch.int32)
    kk = torch.zeros(K, 2, n, ksize_max, device="cuda", dtype=torch.int32)
    ops.roi_coeffs(desc_host, desc_host.cuda(), n, ksize_max, bounds, kk)
    return bounds.cpu().numpy(), kk.cpu().numpy()


def test_device_coefficients_equal_the_host_tables():
    """the FMA-contraction test: windows and every tap of cclip_roi_coeffs against resample_coeffs + the crop slice, for each
    (in, out) pair on both axes.  The descriptors are written by hand so that an axis resizes `in` to exactly `out`."""
    from clip.preprocess_device import ROI_FIELDS, resample_coeffs
    n = 224
    host = {p: resample_coeffs(*p) for p in PAIRS}
    rows = []
    for a, (w, nw) in enumerate(PAIRS):                        # pair a on the horizontal axis, the next pair on the vertical one
        h, nh = PAIRS[(a + 1) % len(PAIRS)]
        left, top = (nw - n + 1) // 2, (nh - n) // 2
        bv = host[(h, nh)][0][top:top + n]
        row0, row1 = int(bv[:, 0].min()), int((bv[:, 0] + bv[:, 1]).max())
        d = dict(src_off=0, src_ld=3 * w, tmp_off=0, w=w, h=h, nw=nw, nh=nh, left=left, top=top, row0=row0, rows=row1 - row0)
        rows.append([d[f] for f in ROI_FIELDS])
    ksize_max = max(v[2] for v in host.values())
    assert ksize_max == 127                                    # 7000 -> 224: the widest window of the list
    bounds, kk = _tables(np.array(rows, dtype=np.int64), n, ksize_max)
    for a, row in enumerate(rows):
        d = dict(zip(ROI_FIELDS, row))
        for axis, (size, out, first) in enumerate(((d["w"], d["nw"], d["left"]), (d["h"], d["nh"], d["top"]))):
            hb, hk, ks = host[(size, out)]
            assert np.array_equal(bounds[a, axis], hb[first:first + n]), (size, out, axis)
            for j in range(n):
                cnt = int(hb[first + j, 1])
                assert np.array_equal(kk[a, axis, j, :cnt], hk[first + j, :cnt]), (size, out, axis, j)


def test_device_coefficients_through_the_descriptor():
    """the same tables for boxes whose geometry comes from roi_descriptors, against plan()"""
    from clip.preprocess_device import plan, roi_descriptors
    n = 224
    sizes = [(640, 298), (61, 224), (224, 224), (1080, 224), (7000, 224), (2, 224), (224, 2), (298, 640)]
    boxes = np.array([[0, 0, w, h] for w, h in sizes], dtype=np.int64)
    z = np.zeros(len(sizes), dtype=np.int64)
    desc, ksize_max, _ = roi_descriptors(boxes, z, 3 * boxes[:, 2], n)
    bounds, kk = _tables(desc, n, ksize_max)
    for a, (w, h) in enumerate(sizes):
        p = plan(w, h, n)
        for axis, (hb, hk) in enumerate(((p["bh"], p["kh"]), (p["bv"], p["kv"]))):
            assert np.array_equal(bounds[a, axis], hb), (w, h, axis)
            for j in range(n):
                assert np.array_equal(kk[a, axis, j, :hb[j, 1]], hk[j, :hb[j, 1]]), (w, h, axis, j)


@pytest.mark.parametrize("n", [32, 224])
def test_regions_are_bit_identical_per_box(n, photo_vga):
    import clip
    pre = clip.DevicePreprocess(n)
    boxes = _vga_boxes(n)
    got = pre.regions(photo_vga, boxes)
    assert got.shape == (len(boxes), 3, n, n) and got.dtype == torch.float32 and got.is_cuda
    want = _host(photo_vga, boxes, n)
    for k, b in enumerate(boxes):
        assert torch.equal(got[k].cpu(), want[k]), (n, b)
    arr = np.asarray(photo_vga)
    assert torch.equal(pre.regions(arr, np.array(boxes)).cpu(), want)                      # uint8 HWC array, int array boxes
    assert torch.equal(pre.regions(torch.from_numpy(arr.copy()).cuda(), boxes).cpu(), want)   # a tensor already on the device
    fl = [(b[0] - 0.4, b[1] - 0.9, b[2] + 0.2, b[3] + 0.7) for b in boxes[2:3] + boxes[7:]]    # floats grow to the pixel box
    grown = [(b[0] - 1, b[1] - 1, b[2] + 1, b[3] + 1) for b in boxes[2:3] + boxes[7:]]
    assert torch.equal(pre.regions(photo_vga, fl).cpu(), _host(photo_vga, grown, n))


@pytest.mark.parametrize("n", [32, 224])
def test_regions_of_a_large_photo(n, photo_big):
    """3000 x 2000: a downscale of about 9 at n = 224 and of 62.5 at n = 32 - inside the limit of 64, so it is supported and
    exact; a 1100 x 1000 box at n = 32 (about 31); and past the limit the documented ValueError."""
    import clip
    from clip.preprocess_device import MAX_DOWNSCALE
    assert MAX_DOWNSCALE == 64
    pre = clip.DevicePreprocess(n)
    boxes = [(0, 0, 3000, 2000)] + ([(1500, 700, 2600, 1700)] if n == 32 else [])
    got = pre.regions(photo_big, boxes)
    want = _host(photo_big, boxes, n)
    for k, b in enumerate(boxes):
        assert torch.equal(got[k].cpu(), want[k]), (n, b)


def test_a_downscale_past_the_limit_raises():
    import clip
    img = np.zeros((2100, 2100, 3), dtype=np.uint8)                                        # 2100 / 32 = 65.6 > 64
    with pytest.raises(ValueError, match="at most 64"):
        clip.DevicePreprocess(32).regions(img, [(0, 0, 40, 40), (0, 0, 2100, 2100)])


def test_many_equals_the_stacked_host_pipeline():
    import clip
    n = 96
    imgs = [_photo(w, h, 20 + i) for i, (w, h) in enumerate(((300, 400), (500, 250), (224, 224), (97, 61)))]
    pre = clip.DevicePreprocess(n)
    want = torch.stack([clip._transform(n)(im) for im in imgs])
    got = pre.many(imgs)
    assert got.shape == (4, 3, n, n) and torch.equal(got.cpu(), want)
    assert torch.equal(got, pre.batch(imgs))
    lists = [[(0, 0, 300, 400), (10, 20, 110, 333)], [(250, 0, 500, 250)], np.array([[0.5, 0.5, 96.5, 96.5], [100, 100, 224, 224]]),
             [(0, 0, 2, 2), (5, 7, 97, 61), (90, 50, 97, 61)]]
    got = pre.many(imgs, lists)
    rounded = [lists[0], lists[1], [(0, 0, 97, 97), (100, 100, 224, 224)], lists[3]]
    want = torch.cat([_host(im, b, n) for im, b in zip(imgs, rounded)])
    assert got.shape == (8, 3, n, n) and torch.equal(got.cpu(), want)
    from PIL import Image
    gray = Image.fromarray(np.random.default_rng(3).integers(0, 256, size=(120, 90), dtype=np.uint8), "L")   # host pipeline rows
    mixed = pre.many([imgs[0], gray, imgs[3]], [lists[0], [(0, 0, 90, 120), (4, 4, 60, 70)], lists[3]])
    want = torch.cat([_host(imgs[0], lists[0], n), _host(gray, [(0, 0, 90, 120), (4, 4, 60, 70)], n), _host(imgs[3], lists[3], n)])
    assert torch.equal(mixed.cpu(), want)
    assert torch.equal(pre.regions(gray, [(4, 4, 60, 70)]).cpu(), _host(gray, [(4, 4, 60, 70)], n))
    with pytest.raises(ValueError, match="image 1: box 0 "):
        pre.many(imgs[:2], [lists[0], [(499, 0, 500, 250)]])


def test_past_the_grid_cap():
    """nine boxes of about 700 x 650 at n = 224: the intermediate has more samples than 4096 work-groups of 256 threads cover
    in one step, and more boxes than the second grid dimension gets - both strided loops of the horizontal pass run."""
    import clip
    from clip.preprocess_device import roi_descriptors
    n = 224
    photo = _photo(2100, 2000, 13)
    boxes = [(x, y, x + 700 - (i % 3), y + 650 + (i // 3)) for i, (x, y) in
             enumerate((x, y) for y in (0, 660, 1340) for x in (0, 701, 1400))]
    z = np.zeros(len(boxes), dtype=np.int64)
    assert roi_descriptors(np.array(boxes), z, z + 6300, n)[2] // 3 > 4096 * 256
    got = clip.DevicePreprocess(n).regions(photo, boxes)
    want = _host(photo, boxes, n)
    for k, b in enumerate(boxes):
        assert torch.equal(got[k].cpu(), want[k]), b


def test_determinism_and_isolation(photo_vga):
    import clip
    n = 64
    pre = clip.DevicePreprocess(n)
    boxes = _vga_boxes(n)
    a, b = pre.regions(photo_vga, boxes), pre.regions(photo_vga, boxes)
    assert torch.equal(a, b)
    perm = np.random.default_rng(1).permutation(len(boxes))
    c = pre.regions(photo_vga, [boxes[i] for i in perm])
    assert torch.equal(c, a[torch.from_numpy(perm).cuda()])
    assert torch.equal(pre.regions(photo_vga, boxes[3:4]), a[3:4])                          # a row does not depend on its neighbours
    assert pre.regions(photo_vga, []).shape == (0, 3, n, n)


def test_through_the_model():
    import clip
    from clip.data import ZeroShotClassifier
    from clip.weights import MODELS, init_state_dict, synthetic_text
    from PIL import Image
    geo = MODELS["test-small"]
    n = geo.image_resolution
    model = clip.build_model(init_state_dict(geo, 3)).cuda().eval()
    rng = np.random.default_rng(9)
    px = rng.integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    for i, (ys, xs) in enumerate((y, x) for y in (slice(0, 240), slice(240, 480)) for x in (slice(0, 320), slice(320, 640))):
        px[ys, xs, i % 3] //= 8                                                             # four quadrants of different tint
        px[ys, xs, (i + 1) % 3] //= (1 + i)
    img = Image.fromarray(px, "RGB")
    boxes = [(10, 10, 300, 230), (330, 5, 630, 235), (20, 250, 310, 470), (330, 250, 640, 480), (0, 0, 640, 480), (100, 100, 102, 102)]
    crops = _host(img, boxes, n).cuda()
    with torch.no_grad():
        want = model.encode_image(crops)
    feats = clip.encode_regions(model, img, boxes)
    assert feats.shape == (len(boxes), geo.embed_dim) and torch.equal(feats, want)
    assert torch.equal(clip.encode_regions(model, img, boxes, preprocess=clip.DevicePreprocess(n), chunk=4)[:4], model.encode_image(crops[:4]))
    head = ZeroShotClassifier(model, synthetic_text(5, geo, 5), ["a", "b", "c", "d", "e"])
    sim, idx, labels = clip.classify_regions(head, img, boxes)
    wsim, widx, wlabels = head(crops)
    assert torch.equal(sim, wsim) and torch.equal(idx, widx) and labels == wlabels
    meta = [("site.jpg", b) for b in boxes]
    index = clip.EmbeddingIndex(torch.empty(0, geo.embed_dim), dtype=torch.float16)
    index.add(clip.encode_regions(model, img, boxes), metadata=meta)
    assert len(index) == len(boxes)
    _, hits = index.search(feats, k=2)
    assert hits[:, 0].tolist() == list(range(len(boxes)))
    assert [index.metadata[i] for i in hits[:, 0].tolist()] == meta


def test_errors(photo_vga):
    import clip
    from cclip_hip import ops
    from clip.preprocess_device import roi_descriptors
    n = 32
    boxes = np.array([[0, 0, 640, 480], [0, 0, 40, 40]], dtype=np.int64)
    z = np.zeros(2, dtype=np.int64)
    desc_np, ksize_max, tmp_bytes = roi_descriptors(boxes, z, z + 3 * 640, n)
    assert ksize_max == 63                                                                  # 640 -> int(32 * 640 / 480) = 42: 2 * ceil(30.5) + 1
    desc_host = torch.from_numpy(desc_np)
    desc = desc_host.cuda()
    bounds = torch.zeros(2, 2, n, 2, device="cuda", dtype=torch.int32)
    small = torch.zeros(2, 2, n, ksize_max - 2, device="cuda", dtype=torch.int32)
    with pytest.raises(RuntimeError, match="cclip_roi_coeffs"):
        ops.roi_coeffs(desc_host, desc, n, ksize_max - 2, bounds, small)
    kk = torch.zeros(2, 2, n, ksize_max, device="cuda", dtype=torch.int32)
    src = torch.zeros(480 * 640 * 3, device="cuda", dtype=torch.uint8)
    tmp = torch.zeros(tmp_bytes, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="cclip_roi_resample_h"):
        ops.roi_resample_h(src, desc_host, desc, n, ksize_max - 2, bounds, small, tmp)
    with pytest.raises(RuntimeError, match="cclip_roi_resample_h"):                         # a source shorter than a box reaches
        ops.roi_resample_h(src[:-1], desc_host, desc, n, ksize_max, bounds, kk, tmp)
    with pytest.raises(RuntimeError, match="cclip_roi_resample_h"):                         # an intermediate shorter than the rows
        ops.roi_resample_h(src, desc_host, desc, n, ksize_max, bounds, kk, tmp[:-1])
    bad = desc_np.copy()
    bad[1, 9] += 1                                                                          # row0 that is not the first window's start
    with pytest.raises(RuntimeError, match="cclip_roi_coeffs"):
        ops.roi_coeffs(torch.from_numpy(bad), desc, n, ksize_max, bounds, kk)
    with pytest.raises(TypeError):
        ops.roi_coeffs(desc_host, desc_host, n, ksize_max, bounds, kk)                      # descriptors on the CPU
    with pytest.raises(TypeError):
        ops.roi_coeffs(desc_host, desc, n, ksize_max, bounds.cpu(), kk)
    with pytest.raises(TypeError):
        ops.roi_resample_h(src.cpu(), desc_host, desc, n, ksize_max, bounds, kk, tmp)
    out = torch.zeros(2, 3, n, n, device="cuda")
    with pytest.raises(TypeError):
        ops.roi_resample_v_norm(tmp, desc_host, desc, n, ksize_max, bounds, kk, (0.5, 0.5, 0.5), (0.2, 0.2, 0.2), out.cpu())
    with pytest.raises(ValueError, match="box 1 "):
        clip.DevicePreprocess(n).regions(photo_vga, [(0, 0, 10, 10), (700, 0, 800, 50)])


def test_classify_regions_script_synthetic():
    """`scripts/classify_regions.py --synthetic`: exit 0, exactly one JSON line per box, and the labels and
    probabilities of each line equal the two zero-shot heads on the host-preprocessed crops of the same seeded inputs."""
    K = 7
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "classify_regions.py"), "--synthetic", "--n_boxes", str(K)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == K, r.stdout[-2000:]
    recs = [json.loads(ln) for ln in lines]
    keys = {"box", "label", "score", "caption_type", "caption_type_prob", "violation_type", "violation_type_prob"}
    assert all(set(rec) == keys for rec in recs)

    sys.path[:0] = [os.path.join(ROOT, "scripts")]
    try:
        import _common as C
        import classify_regions as S
        from describe_images import SYNTHETIC_TYPES, SYNTHETIC_VIOLATIONS
    finally:
        sys.path.pop(0)
    import clip
    from clip.data import ZeroShotClassifier
    from clip.preprocess_device import normalize_boxes
    args = S.build_parser().parse_args(["--synthetic"])
    image, det = S.synthetic_inputs(K, args.seed)
    assert [rec["box"] for rec in recs] == det["boxes"]
    assert [rec["label"] for rec in recs] == det["labels"] and [rec["score"] for rec in recs] == det["scores"]
    model, _ = clip.load(args.clip_synthetic, device="cuda:0", jit=False)
    model.eval()
    tokenize = C.get_tokenize(model)
    crops = _host(image, normalize_boxes(det["boxes"], *image.size), model.visual.input_resolution).cuda()
    t_sim, _, t_lab = ZeroShotClassifier(model, tokenize(list(SYNTHETIC_TYPES)), list(SYNTHETIC_TYPES.values()))(crops)
    v_sim, _, v_lab = ZeroShotClassifier(model, tokenize(SYNTHETIC_VIOLATIONS), SYNTHETIC_VIOLATIONS)(crops)
    for k, rec in enumerate(recs):
        assert 0.0 <= rec["caption_type_prob"] <= 1.0 and 0.0 <= rec["violation_type_prob"] <= 1.0
        assert (rec["caption_type"], rec["violation_type"]) == (t_lab[k], v_lab[k]), k
        assert rec["caption_type_prob"] == round(t_sim[k].max().item(), 5) and rec["violation_type_prob"] == round(v_sim[k].max().item(), 5)
