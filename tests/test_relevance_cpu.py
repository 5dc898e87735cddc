"""Relevance maps without a GPU: the display helpers of clip.explain against the reference's formulas, and the float64
restatement of the reference's interpret() (attention.py:14-69) that tests/test_relevance_gpu.py measures the
HIP path against.  The restatement is pinned here: its logits are the oracle's, start_layer = L-1 is the closed form
I + C_{L-1}, and the top-down right-multiplied rollout (what the backward computes) is the reference's bottom-up one."""
import pytest
import torch
import torch.nn.functional as F

from oracle import clip_oracle as O


# ------------------------------------------------------------------------------------------------------------------------
# float64 restatement of interpret(): CLIP's forward with every block's attention probabilities kept (retain_grad), the
# score sum_i logits_per_image[i, i], one backward, then the reference's rollout
# ------------------------------------------------------------------------------------------------------------------------
def _ln(x, sd, key):
    return F.layer_norm(x, (x.shape[-1],), sd[key + ".weight"], sd[key + ".bias"], 1e-5)


def _block(x, p, sd, heads, mask, probs):
    n, t, d = x.shape
    dh = d // heads
    qkv = _ln(x, sd, p + "ln_1") @ sd[p + "attn.in_proj_weight"].t() + sd[p + "attn.in_proj_bias"]
    q, k, v = (z.reshape(n, t, heads, dh).transpose(1, 2) for z in qkv.split(d, dim=-1))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    if mask is not None:
        s = s + mask
    P = torch.softmax(s, dim=-1)
    P.retain_grad()
    probs.append(P)
    a = (P @ v).transpose(1, 2).reshape(n, t, d)
    x = x + a @ sd[p + "attn.out_proj.weight"].t() + sd[p + "attn.out_proj.bias"]
    h = _ln(x, sd, p + "ln_2") @ sd[p + "mlp.c_fc.weight"].t() + sd[p + "mlp.c_fc.bias"]
    h = O.quick_gelu(h) @ sd[p + "mlp.c_proj.weight"].t() + sd[p + "mlp.c_proj.bias"]
    return x + h


def forward64(sd, image, text):
    """(logits_per_image, image-tower probabilities per block, text-tower probabilities per block), float64."""
    cfg = O.infer_config(sd)
    x = F.conv2d(image.double(), sd["visual.conv1.weight"], stride=cfg["vision_patch_size"])
    n, w = x.shape[0], x.shape[1]
    x = x.reshape(n, w, -1).permute(0, 2, 1)
    x = torch.cat([sd["visual.class_embedding"].expand(n, 1, w), x], dim=1) + sd["visual.positional_embedding"]
    x = _ln(x, sd, "visual.ln_pre").detach().requires_grad_(True)       # (a leaf: the graph reaches every P)
    pi = []
    for i in range(cfg["vision_layers"]):
        x = _block(x, f"visual.transformer.resblocks.{i}.", sd, cfg["vision_heads"], None, pi)
    fi = _ln(x[:, 0], sd, "visual.ln_post") @ sd["visual.proj"]
    tok = text.long()
    x = (sd["token_embedding.weight"][tok] + sd["positional_embedding"][: tok.shape[1]]).detach().requires_grad_(True)
    mask = O.causal_mask(tok.shape[1]).double()
    pt = []
    for i in range(cfg["transformer_layers"]):
        x = _block(x, f"transformer.resblocks.{i}.", sd, cfg["transformer_heads"], mask, pt)
    ft = _ln(x, sd, "ln_final")[torch.arange(n), tok.argmax(dim=-1)] @ sd["text_projection"]
    fi = fi / fi.norm(dim=1, keepdim=True)
    ft = ft / ft.norm(dim=1, keepdim=True)
    return sd["logit_scale"].exp() * fi @ ft.t(), pi, pt


def cams(probs):
    """C_l = mean over heads of clamp(P_l * dP_l, min=0), [N, T, T] per block (attention.py:38-45)."""
    return [(P.detach() * P.grad).clamp(min=0).mean(dim=1) for P in probs]


def rollout(cs, start_layer, order="bottom_up"):
    """attention.py:27-46: R = I; R <- R + C_l R for the blocks l >= start (start -1: the last block), bottom-up.
    order="top_down": R <- R + R C_l from the last block down - the order the backward visits the blocks in."""
    L = len(cs)
    s = L - 1 if start_layer == -1 else start_layer
    n, t = cs[0].shape[0], cs[0].shape[-1]
    R = torch.eye(t, dtype=cs[0].dtype).expand(n, t, t).clone()
    if order == "bottom_up":
        for i in range(L):
            if i >= s:
                R = R + torch.bmm(cs[i], R)
    else:
        for i in range(L - 1, -1, -1):
            if i >= s:
                R = R + torch.bmm(R, cs[i])
    return R


def ref_interpret(sd, image, text, start_layer=-1, start_layer_text=-1, order="bottom_up"):
    """float64 interpret() on pairs (image i, text i): (R_text [N, T, T], R_image [N, T_img, T_img], logits)."""
    sd64 = {k: v.detach().double() for k, v in sd.items()}
    with torch.enable_grad():
        logits, pi, pt = forward64(sd64, image, text)
        logits.diagonal().sum().backward()
    return rollout(cams(pt), start_layer_text, order), rollout(cams(pi), start_layer, order), logits.detach()


def _fixture(name="test-tiny", n=3, seed=11):
    from clip.weights import MODELS, init_state_dict, synthetic_images, synthetic_text
    geo = MODELS[name]
    return init_state_dict(geo, seed), synthetic_images(n, geo, seed + 1), synthetic_text(n, geo, seed + 2)


# ------------------------------------------------------------------------------------------------------------------------
def test_restatement_logits_match_oracle():
    sd, img, txt = _fixture()
    _, _, logits = ref_interpret(sd, img, txt)
    li, _ = O.clip_forward(sd, img, txt)
    assert (logits - li.double()).abs().max().item() < 1e-5


@pytest.mark.parametrize("name", ["test-tiny", "test-small"])
def test_last_block_is_closed_form(name):
    sd, img, txt = _fixture(name)
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.enable_grad():
        logits, pi, pt = forward64(sd64, img, txt)
        logits.diagonal().sum().backward()
    for probs in (pi, pt):
        cs = cams(probs)
        L = len(cs)
        eye = torch.eye(cs[0].shape[-1], dtype=torch.float64)
        for start in (-1, L - 1):
            assert torch.equal(rollout(cs, start), eye + cs[L - 1])
        assert (cs[L - 1] >= 0).all() and cs[L - 1].abs().sum() > 0


@pytest.mark.parametrize("start", [-1, 0, 1])
def test_top_down_equals_bottom_up(start):
    sd, img, txt = _fixture("test-small")
    rt_b, ri_b, _ = ref_interpret(sd, img, txt, start, start)
    rt_t, ri_t, _ = ref_interpret(sd, img, txt, start, start, order="top_down")
    assert (rt_b - rt_t).abs().max().item() < 1e-12
    assert (ri_b - ri_t).abs().max().item() < 1e-12


def test_text_rows_past_eot_stay_identity():
    """Rows and columns after each caption's EOT never receive relevance (causal tower, EOT pooling): what lets the packed
    text tower leave them as they came."""
    sd, img, txt = _fixture("test-small")
    rt, _, _ = ref_interpret(sd, img, txt, 0, 0)
    T = txt.shape[1]
    for b in range(txt.shape[0]):
        e = int(txt[b].long().argmax())
        eye = torch.eye(T, dtype=torch.float64)
        assert torch.equal(rt[b, e + 1:], eye[e + 1:])
        assert torch.equal(rt[b, :, e + 1:], eye[:, e + 1:])


# ------------------------------------------------------------------------------------------------------------------------
def test_image_relevance_map_matches_reference_formula():
    from clip import image_relevance_map
    g = torch.Generator().manual_seed(3)
    r = torch.rand(2, 49, generator=g)
    got = image_relevance_map(r, 224)
    assert got.shape == (2, 224, 224)
    for i in range(2):
        # attention.py:88-92
        x = r[i].reshape(1, 1, 7, 7)
        x = F.interpolate(x, size=224, mode="bilinear").reshape(224, 224).numpy()
        x = (x - x.min()) / (x.max() - x.min())
        assert abs(got[i].numpy() - x).max() < 1e-6
    one = image_relevance_map(r[0], 112)
    assert one.shape == (112, 112) and one.min() == 0 and one.max() == 1
    assert image_relevance_map(torch.ones(49)).abs().max() == 0          # a constant map: zeros, not NaN


def test_text_token_scores_match_reference_formula():
    from clip import text_token_scores
    g = torch.Generator().manual_seed(4)
    R = torch.rand(2, 16, 16, generator=g)
    tok = torch.zeros(2, 16, dtype=torch.int32)
    tok[0, :6] = torch.tensor([510, 7, 8, 9, 10, 511])
    tok[1, :3] = torch.tensor([510, 7, 511])
    got = text_token_scores(R, tok)
    for b in range(2):
        cls = tok[b].argmax(dim=-1)                                    # attention.py:115-117
        r = R[b][cls, 1:cls]
        ref = (r / r.sum()).flatten()
        assert torch.allclose(got[b], ref, atol=0, rtol=1e-6)
        assert abs(got[b].sum().item() - 1) < 1e-6
    assert torch.equal(text_token_scores(R[0], tok[0]), got[0])


def test_interpret_is_exported():
    import clip
    from clip.explain import interpret
    assert clip.interpret is interpret
    import inspect
    assert list(inspect.signature(interpret).parameters) == ["image", "texts", "model", "device", "start_layer",
                                                             "start_layer_text"]
