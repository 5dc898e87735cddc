"""The argument contract of the embedding-analysis wrappers of cclip_hip/ops.py (retrieval, range search, lm_head scoring, the
cache classifier, k-means, coreset, the HDBSCAN spanning tree, the linear probe, t-SNE, label spreading, concept codes): one
table of (wrapper, violation) -> exception class.  Every row starts from the smallest legal call (3 rows, D = 32, k = 2, C = 2,
nnz = 4), breaks one argument (the precedence rows: two), expects exactly that class and then checks that no tensor argument -
the caller's outputs hold a fill of 7 - was written.  The order the rows pin: cuda before dtype before shape over all the
tensors of a call, then the size limits, then alignment.  Nothing here launches a kernel except the legal calls and the
one-row-view tests at the end."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, V, N_ = TypeError, ValueError, NotImplementedError
D0 = 32


def rows16(n, D=D0, dtype=torch.bfloat16, seed=0):
    x = torch.randn(n, max(D, 1), generator=torch.Generator().manual_seed(seed + 31 * n + D))
    x = (x / x.norm(dim=1, keepdim=True)).to(dtype).cuda()
    return x if D else torch.zeros(n, 8, dtype=dtype, device="cuda")[:, :0]      # D = 0: a legal stride, so that only D is wrong


def f32(*shape, fill=7.0):
    return torch.full(shape, fill, dtype=torch.float32, device="cuda")


def i32(*shape, fill=7, dtype=torch.int32):
    return torch.full(shape, fill, dtype=dtype, device="cuda")


def csr():
    """3 rows, nnz = 4: a symmetric graph 0-1, 0-2"""
    return dict(offsets=torch.tensor([0, 2, 3, 4], device="cuda"), cols=torch.tensor([1, 2, 0, 0], dtype=torch.int32, device="cuda"),
                vals=torch.tensor([0.5, 0.25, 0.5, 0.25], device="cuda"))


def layout():
    from cclip_hip import ops
    _, class_off, class_len = ops.cache_layout([0, 1, 0], 2)                     # two segments of 16 rows: Np = 32
    return class_off, class_len


# ------------------------------------------------------------------------------------------------------------------------
# the smallest legal arguments of every wrapper, as a dict, and how the dict is passed
# ------------------------------------------------------------------------------------------------------------------------
def b_topk(D=D0):
    return dict(q=rows16(3, D), g=rows16(3, D, seed=1), k=2, out_scores=f32(3, 2), out_index=i32(3, 2))


def b_range(D=D0):
    return dict(q=rows16(3, D), g=rows16(3, D, seed=1), threshold=0.1)


def b_lm(D=D0):
    return dict(x16=rows16(3, D), w16=rows16(3, D, seed=1), labels_i32=i32(3, fill=1), logp=f32(3), lse=f32(3), pred=i32(3),
                pred_logit=f32(3))


def b_cache(D=D0):
    class_off, class_len = layout()
    return dict(q=rows16(3, D), g=rows16(32, D, seed=1), class_off=class_off, class_len=class_len, beta=5.5, exclude=i32(3, fill=-1),
                out=f32(3, 2))


def b_cache_bwd(D=D0):
    a = b_cache(D)
    a.update(dA=f32(3, 2, fill=0.5), out=f32(32, D))
    return a


def b_assign(D=D0):
    return dict(x=rows16(3, D), c=rows16(3, D, seed=1), out_assign=i32(3), out_best=f32(3), out_second=f32(3))


def b_update(D=D0):
    return dict(x=rows16(3, D), assign=i32(3, fill=1), K=2, prev_c=rows16(2, D, seed=1), out_c=torch.full((2, D), 7.0, device="cuda").bfloat16(),
                out_norm=f32(2))


def b_cstep(D=D0):
    return dict(x=rows16(3, D), mind=f32(3, fill=float("inf")), owner=i32(3, fill=-1), partial_out=i32(1, dtype=torch.int64), centre=0,
                partial_in=None, weight=f32(3, fill=1.0), out_pick=i32(1), out_radius=f32(1))


def b_cscan(D=D0):
    a = b_cstep(D)
    a.update(centre=None, scan_only=True, partial_in=i32(1, dtype=torch.int64), out_pick=None, out_radius=None)
    return a


def b_cgreedy(D=D0):
    return dict(x=rows16(3, D), mind=f32(3, fill=float("inf")), owner=i32(3, fill=-1), m=2, first=0, workspace=i32(2, 1, dtype=torch.int64),
                weight=f32(3, fill=1.0), out_picks=i32(2), out_radius=f32(2))


def b_mreach(D=D0):
    return dict(x=rows16(3, D), core=f32(3, fill=0.5), comp=torch.arange(3, dtype=torch.int32, device="cuda"), out=i32(3, dtype=torch.int64))


def b_mst(D=D0):
    from cclip_hip import ops
    return dict(x=rows16(3, D), core=f32(3, fill=0.5), workspace=i32((ops.mst_workspace(3) + 7) // 8, dtype=torch.int64))


def b_pfwd(D=D0):
    return dict(x=rows16(3, D), W=f32(2, D, fill=0.25), bias=f32(2, fill=0.5), labels=i32(3, fill=1), row_weight=f32(3, fill=1.0),
                o_lse=f32(3), o_loss=f32(3), o_pred=i32(3), o_logits=f32(3, 2))


def b_pbwd(D=D0):
    return dict(x=rows16(3, D), W=f32(2, D, fill=0.25), bias=f32(2, fill=0.5), labels=i32(3, fill=1), lse=f32(3, fill=1.0), scale=0.5, l2=0.01,
                row_weight=f32(3, fill=1.0), loss=f32(3, fill=0.5), o_dW=f32(2, D), o_db=f32(2), o_obj=f32(1))


def b_taff(D=D0):
    return dict(scores=torch.tensor([[0.9, 0.5, 0.1]] * 3, device="cuda"), perplexity=2.0, out_P=f32(3, 3), out_beta=f32(3))


def b_trep(D=D0):
    from cclip_hip import ops
    return dict(y=f32(3, 2, fill=0.5) * torch.arange(1, 4, device="cuda")[:, None], out_zrow=f32(3), out_rep=f32(3, 2), out_z=f32(1),
                workspace=f32(ops.tsne_repulsion_workspace(3) // 4))


def b_tstep(D=D0):
    y = f32(3, 2, fill=0.5) * torch.arange(1, 4, device="cuda")[:, None]
    return dict(y=y, vel=f32(3, 2, fill=0.0), gains=f32(3, 2, fill=1.0), **csr(), rep=f32(3, 2, fill=0.1), z=f32(1, fill=2.0), exaggeration=1.0,
                momentum=0.8, learning_rate=200.0, min_gain=0.01, out_y=f32(3, 2), out_kl=f32(3))


def b_lnorm(D=D0):
    return dict(**csr(), out_deg=f32(3), out_vals=f32(4))


def b_lstep(D=D0):
    return dict(F=f32(3, 2, fill=0.5), labels=i32(3, fill=1), **csr(), alpha=0.9, class_weight=f32(2, fill=1.0), out_F=f32(3, 2), out_delta=f32(3))


def b_lfin(D=D0):
    return dict(F=f32(3, 2, fill=0.5), out_dist=f32(3, 2), out_pred=i32(3), out_conf=f32(3), out_cert=f32(3))


def b_concept(D=D0):
    from cclip_hip import ops
    return dict(x=rows16(3, D), c=rows16(3, D, seed=1), l1=0.1, eta=0.5, iters=2, out_w=f32(3, 4)[:, :3],
                workspace=f32(max(ops.concept_codes_workspace(3, 3, D) // 4, 1)))


def _probe_fwd(o, a):
    a = dict(a)
    out = tuple(a.pop(k) for k in ("o_lse", "o_loss", "o_pred", "o_logits"))
    return o.probe_forward(**a, out=out)


def _probe_bwd(o, a):
    a = dict(a)
    out = tuple(a.pop(k) for k in ("o_dW", "o_db", "o_obj"))
    return o.probe_backward(**a, out=out)


def _kw(name):
    return lambda o, a: getattr(o, name)(**a)


# what a caller-provided tensor answers to (a host tensor, a non-tensor, a wrong dtype, a wrong shape, a non-contiguous one);
# None: not a row (a one-element tensor is always contiguous; a view is accepted)
ALL_V = (V, V, V, V, V)            # outputs and key buffers: every violation is a ValueError
CUDA_T = (T, T, T, V, V)           # t-SNE, label spreading, CSR: host and dtype are TypeErrors
STATE = (T, T, V, V, V)            # coreset / mreach state vectors: only the host tensor is a TypeError
REQ = (T, T, T, V, V)           # the cache wrappers' tensors
AUX_KINDS = ("host", "nontensor", "dtype", "shape", "noncontig")

# wrapper -> (call, base, 16-bit operands, {operand: class of a non-tensor}, class of a wrong / mixed dtype, class of D = 0 ("C": the
#             C entry's refusal), {tensor: classes}, {float: violations})
def _cclip_error():
    from cclip_hip._lib import CclipError
    return CclipError


SPEC = {
    "similarity_topk": (_kw("similarity_topk"), b_topk, ("q", "g"), {}, T, "C",
                        # a wrong-shaped or non-contiguous out_scores / out_index was one bare assert before the wrappers shared
                        # `_out`: THE one check of this table that differs from the parent commit, where these four rows raised
                        # AssertionError (and nothing at all under python -O)
                        {"out_scores": (T, T, T, V, V), "out_index": (T, T, T, V, V)}, {}),
    "similarity_range": (_kw("similarity_range"), b_range, ("q", "g"), {}, T, "C", {}, {"threshold": ("nan",)}),
    "lm_head_score": (_kw("lm_head_score"), b_lm, ("x16", "w16"), {}, V, N_,
                      {"labels_i32": (T, T, V, V, V), "logp": ALL_V, "lse": ALL_V, "pred": ALL_V,
                       "pred_logit": ALL_V}, {}),
    "cache_affinity": (_kw("cache_affinity"), b_cache, ("q", "g"), {}, T, N_, {"exclude": REQ, "out": REQ},
                       {"beta": ("nan", "inf", "-inf")}),
    "cache_affinity_backward": (_kw("cache_affinity_backward"), b_cache_bwd, ("q", "g"), {}, T, N_, {"exclude": REQ, "dA": REQ, "out": REQ},
                                {"beta": ("nan", "inf", "-inf")}),
    "kmeans_assign": (_kw("kmeans_assign"), b_assign, ("x", "c"), {}, T, N_, {"out_assign": ALL_V, "out_best": ALL_V, "out_second": ALL_V}, {}),
    "kmeans_update": (_kw("kmeans_update"), b_update, ("x", "prev_c"), {}, T, N_,
                      {"assign": (T, T, T, V, None), "out_c": (V, V, V, V, None), "out_norm": ALL_V}, {}),
    "coreset_step": (_kw("coreset_step"), b_cstep, ("x",), {}, T, N_,
                     {"mind": STATE, "owner": STATE, "weight": STATE, "partial_out": (V, V, V, V, None), "out_pick": (V, V, V, V, None),
                      "out_radius": (V, V, V, V, None)}, {}),
    "coreset_step/scan_only": (_kw("coreset_step"), b_cscan, ("x",), {}, T, N_, {"partial_in": (V, V, V, V, None)}, {}),
    "coreset_greedy": (_kw("coreset_greedy"), b_cgreedy, ("x",), {}, T, N_,
                       {"mind": STATE, "owner": STATE, "weight": STATE, "workspace": ALL_V, "out_picks": ALL_V, "out_radius": ALL_V}, {}),
    "mreach_nearest": (_kw("mreach_nearest"), b_mreach, ("x",), {"x": T}, T, N_, {"core": STATE, "comp": STATE, "out": ALL_V}, {}),
    "mst_boruvka": (_kw("mst_boruvka"), b_mst, ("x",), {"x": T}, T, N_, {"core": STATE, "workspace": (V, V, V, None, V)}, {}),
    "probe_forward": (_probe_fwd, b_pfwd, ("x",), {"x": T}, T, N_,
                      {"W": (T, T, T, V, V), "bias": ALL_V, "labels": ALL_V, "row_weight": ALL_V, "o_lse": ALL_V, "o_loss": ALL_V, "o_pred": ALL_V,
                       "o_logits": ALL_V}, {}),
    "probe_backward": (_probe_bwd, b_pbwd, ("x",), {"x": T}, T, N_,
                       {"W": (T, T, T, V, V), "bias": ALL_V, "labels": ALL_V, "row_weight": ALL_V, "lse": ALL_V, "loss": ALL_V, "o_dW": ALL_V,
                        "o_db": ALL_V, "o_obj": (V, V, V, V, None)}, {"scale": ("nan", "inf", "-inf", "neg"), "l2": ("nan", "inf", "-inf", "neg")}),
    "tsne_affinities": (_kw("tsne_affinities"), b_taff, (), {}, T, N_, {"scores": (T, T, T, None, None), "out_P": ALL_V, "out_beta": ALL_V},
                        {"perplexity": ("nan", "inf", "-inf", "neg")}),
    "tsne_repulsion": (_kw("tsne_repulsion"), b_trep, (), {}, T, N_,
                       {"y": CUDA_T, "out_zrow": ALL_V, "out_rep": ALL_V, "out_z": (V, V, V, V, None), "workspace": (T, T, T, None, V)}, {}),
    "tsne_step": (_kw("tsne_step"), b_tstep, (), {}, T, N_,
                  {"y": CUDA_T, "vel": CUDA_T, "gains": CUDA_T, "rep": CUDA_T, "offsets": CUDA_T, "cols": CUDA_T, "vals": CUDA_T,
                   "z": (T, T, T, V, None), "out_y": ALL_V, "out_kl": ALL_V},
                  {n: ("nan", "inf", "-inf", "neg") for n in ("exaggeration", "momentum", "learning_rate", "min_gain")}),
    "label_graph_normalize": (_kw("label_graph_normalize"), b_lnorm, (), {}, T, N_,
                              {"offsets": CUDA_T, "cols": CUDA_T, "vals": CUDA_T, "out_deg": ALL_V, "out_vals": ALL_V}, {}),
    "label_spread_step": (_kw("label_spread_step"), b_lstep, (), {}, T, N_,
                          {"F": CUDA_T, "labels": CUDA_T, "class_weight": CUDA_T, "offsets": CUDA_T, "cols": CUDA_T, "vals": CUDA_T, "out_F": ALL_V,
                           "out_delta": ALL_V}, {"alpha": ("nan", "inf", "-inf", "neg")}),
    "label_spread_finish": (_kw("label_spread_finish"), b_lfin, (), {}, T, N_,
                            {"F": CUDA_T, "out_dist": ALL_V, "out_pred": ALL_V, "out_conf": ALL_V, "out_cert": ALL_V}, {}),
    "concept_codes": (_kw("concept_codes"), b_concept, ("x", "c"), {}, T, N_,
                      {"out_w": (V, V, V, V, None), "workspace": (V, V, V, None, V)}, {"l1": ("nan", "inf", "-inf", "neg"), "eta": ("nan", "inf", "-inf", "neg")}),
}
WORKSPACES = {"mst_boruvka": "workspace", "tsne_repulsion": "workspace", "concept_codes": "workspace"}
FLOATS = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf"), "neg": -0.5}


def mutate(a, kind, name):
    """break argument `name` of the legal arguments `a` in one way"""
    if kind == "set":
        return a.update(name)
    t = a[name]
    if kind in FLOATS:
        a[name] = FLOATS[kind]
    elif kind == "host":
        a[name] = t.cpu()
    elif kind == "device":
        a[name] = t.to("cuda:1")
    elif kind == "cuda":
        a[name] = t.cuda()
    elif kind == "nontensor":
        a[name] = "nope"
    elif kind == "dtype":
        a[name] = t.to(torch.float64 if t.dtype == torch.float32 else torch.float32)
    elif kind == "mixed":
        a[name] = t.to(torch.float16)
    elif kind == "rank":
        a[name] = t[0]
    elif kind == "rank3":
        a[name] = t[None]
    elif kind == "stride2":
        a[name] = t.repeat_interleave(2, dim=1)[:, ::2]
    elif kind == "zero":
        a[name] = t[:0]
    elif kind in ("ldpad", "offset"):                            # a row stride of D + 4 elements; a base address one element off
        pad, first = (4, 0) if kind == "ldpad" else (8, 1)
        buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
        buf[:, first:first + t.shape[1]] = t
        a[name] = buf[:, first:first + t.shape[1]]
    elif kind == "shape":
        a[name] = torch.cat([t, t])
    elif kind == "noncontig":
        a[name] = torch.stack([t, t], -1)[..., 0]
    elif kind == "short":
        a[name] = t[:-1]
    elif kind == "wide":
        a[name] = rows16(t.shape[0], 64, seed=1)
    else:
        raise AssertionError(kind)


def table():
    out = []
    for w, (call, base, ops16, nontensor, dtype_cls, d0_cls, aux, floats) in SPEC.items():
        for n in ops16:
            out += [(w, [("host", n)], T), (w, [("dtype", n)], dtype_cls), (w, [("rank", n)], V), (w, [("stride2", n)], V), (w, [("zero", n)], V),
                    (w, [("ldpad", n)], V), (w, [("offset", n)], V)]
            out.append((w, [("nontensor", n)], T))
            if len(ops16) == 2:
                out.append((w, [("mixed", n)], dtype_cls))
        if ops16:
            out += [(w, [("D", 48)], N_), (w, [("D", 1056)], N_), (w, [("D", 0)], d0_cls)]
        if len(ops16) == 2:
            out.append((w, [("wide", ops16[1])], V))
        for n, classes in aux.items():
            out += [(w, [(kind, n)], cls) for kind, cls in zip(AUX_KINDS, classes) if cls is not None]
        if w in WORKSPACES:
            out.append((w, [("short", WORKSPACES[w])], V))
        for n, kinds in floats.items():
            out += [(w, [(kind, n)], V) for kind in kinds]
    # arguments with rules of their own
    for w in ("cache_affinity", "cache_affinity_backward"):
        for n in ("class_off", "class_len"):
            out += [(w, [("cuda", n)], T), (w, [("nontensor", n)], T), (w, [("dtype", n)], T), (w, [("rank3", n)], V), (w, [("shape", n)], V)]
    out += [("similarity_topk", [("set", {"k": 0})], V), ("similarity_topk", [("set", {"k": 65})], V), ("similarity_topk", [("set", {"k": 4})], V),
            ("tsne_affinities", [("rank", "scores")], V), ("tsne_affinities", [("stride2", "scores")], V), ("tsne_affinities", [("zero", "scores")], V),
            ("kmeans_update", [("set", {"K": 3})], V), ("probe_forward", [("rank", "W")], V), ("tsne_repulsion", [("rank", "y")], V),
            ("tsne_step", [("rank", "y")], V), ("kmeans_update", [("stride2", "out_c")], V),
            ("concept_codes", [("stride2", "out_w")], V), ("concept_codes", [("offset", "out_w")], V),
            ("concept_codes", [("set", {"iters": -1})], V), ("concept_codes", [("set", {"iters": 1.5})], V),
            ("coreset_step", [("set", {"centre": 3})], V), ("coreset_greedy", [("set", {"m": 4})], V), ("coreset_greedy", [("set", {"first": 3})], V)]
    # two violations at once: which one answers (cuda before dtype before shape before limits before alignment, over all the
    # operands of a wrapper)
    out += [
        ("similarity_topk", [("dtype", "q"), ("host", "q")], T), ("similarity_topk", [("dtype", "q"), ("rank", "q")], T),
        ("similarity_topk", [("D", 48), ("offset", "q")], N_), ("similarity_topk", [("offset", "q"), ("host", "g")], T),
        ("similarity_topk", [("D", 48), ("set", {"k": 0})], V), ("similarity_topk", [("offset", "q"), ("mixed", "g")], V),
        ("similarity_range", [("D", 48), ("nan", "threshold")], N_), ("similarity_range", [("offset", "g"), ("nan", "threshold")], V),
        ("lm_head_score", [("dtype", "x16"), ("host", "w16")], T), ("lm_head_score", [("D", 48), ("host", "labels_i32")], T),
        ("lm_head_score", [("D", 48), ("shape", "labels_i32")], V), ("lm_head_score", [("offset", "x16"), ("shape", "logp")], V),
        ("lm_head_score", [("D", 48), ("dtype", "logp")], N_),
        ("cache_affinity", [("dtype", "exclude"), ("shape", "exclude")], T), ("cache_affinity", [("D", 48), ("nan", "beta")], V),
        ("cache_affinity", [("offset", "q"), ("cuda", "class_off")], T), ("cache_affinity", [("offset", "q"), ("dtype", "out")], V),
        ("cache_affinity_backward", [("D", 48), ("host", "dA")], N_), ("cache_affinity_backward", [("shape", "exclude"), ("dtype", "dA")], V),
        ("kmeans_assign", [("mixed", "c"), ("offset", "c")], T), ("kmeans_assign", [("D", 48), ("shape", "out_assign")], N_),
        ("kmeans_assign", [("D", 48), ("zero", "c")], V),
        ("kmeans_update", [("offset", "x"), ("host", "assign")], V), ("kmeans_update", [("dtype", "assign"), ("shape", "assign")], T),
        ("coreset_step", [("offset", "x"), ("host", "mind")], T), ("coreset_step", [("D", 48), ("host", "mind")], N_),
        ("coreset_step", [("host", "mind"), ("dtype", "mind")], T), ("coreset_step", [("offset", "x"), ("shape", "partial_out")], V),
        ("mreach_nearest", [("offset", "x"), ("host", "core")], T), ("mreach_nearest", [("offset", "x"), ("host", "comp")], V),
        ("mreach_nearest", [("D", 48), ("host", "core")], N_),
        ("probe_forward", [("D", 48), ("host", "W")], T), ("probe_forward", [("D", 48), ("shape", "bias")], N_),
        ("probe_forward", [("dtype", "x"), ("rank", "x")], T), ("probe_backward", [("offset", "x"), ("nan", "scale")], V),
        ("tsne_step", [("host", "offsets"), ("dtype", "offsets")], T), ("tsne_step", [("dtype", "cols"), ("shape", "cols")], T),
        ("tsne_step", [("shape", "vals"), ("host", "z")], V), ("tsne_step", [("nan", "momentum"), ("host", "vel")], V),
        ("tsne_step", [("dtype", "y"), ("shape", "y")], T),
        ("label_spread_step", [("host", "labels"), ("dtype", "labels")], T), ("label_spread_step", [("dtype", "labels"), ("shape", "labels")], T),
        ("label_spread_step", [("shape", "cols"), ("host", "labels")], V), ("label_spread_step", [("nan", "alpha"), ("host", "class_weight")], T),
        ("concept_codes", [("nan", "l1"), ("dtype", "out_w")], V), ("concept_codes", [("D", 48), ("nan", "l1")], N_),
    ]
    return out


# a tensor on another device than the first operand's.  The second operand of a pair and the probe's W are operands (TypeError),
# every other tensor a ValueError; the tensors that define the call's device, and those whose device the wrappers do not
# compare (g of similarity_topk / similarity_range, w16 and labels_i32 of lm_head_score), have no row
DEFINES_DEVICE = {"x", "q", "x16", "y", "F", "scores", "labels_i32"}
SECOND_OPERAND = {"kmeans_assign": "c", "kmeans_update": "prev_c", "cache_affinity": "g", "cache_affinity_backward": "g", "concept_codes": "c",
                  "probe_forward": "W", "probe_backward": "W"}


def device_rows():
    out = [(w, [("device", n)], T) for w, n in SECOND_OPERAND.items()]
    for w, spec in SPEC.items():
        out += [(w, [("device", n)], V) for n in spec[6] if n not in DEFINES_DEVICE and n != SECOND_OPERAND.get(w)
                and not (w == "label_graph_normalize" and n == "offsets")]
    return out


TWO_GPUS = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")


def _id(row):
    w, muts, cls = row
    return w + "-" + "+".join(f"{k}:{n if not isinstance(n, dict) else ','.join(f'{a}={b}' for a, b in n.items())}" for k, n in muts)


def arguments(w, muts):
    base = SPEC[w][1]
    D = next((n for k, n in muts if k == "D"), D0)
    a = base(D)
    for kind, name in muts:
        if kind != "D":
            mutate(a, kind, name)
    return a


@pytest.mark.parametrize("row", table() + [pytest.param(r, marks=TWO_GPUS) for r in device_rows()],
                         ids=lambda r: _id(r))
def test_violation_raises_the_class_and_writes_nothing(row):
    from cclip_hip import ops
    w, muts, cls = row
    if cls == "C":                                           # the C entry's refusal: D = 0 passes similarity_topk's Python checks
        cls = _cclip_error()
    a = arguments(w, muts)
    before = {k: v.clone() for k, v in a.items() if isinstance(v, torch.Tensor)}
    with pytest.raises(cls) as info:
        SPEC[w][0](ops, a)
    assert type(info.value) is cls, f"{type(info.value).__name__}: {info.value}"
    torch.cuda.synchronize()
    for k, v in before.items():
        assert a[k].dtype == v.dtype and torch.equal(_bits(a[k]), _bits(v)), \
            f"{k} was written by a refused call"


@pytest.mark.parametrize("w", list(SPEC))
def test_the_legal_call_is_accepted(w):
    """the rows above start from these arguments: each must be a call the wrapper takes"""
    from cclip_hip import ops
    SPEC[w][0](ops, SPEC[w][1]())
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------
# a one-row view's row stride is free
# ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().cpu().reshape(-1).view(torch.uint8)


def test_one_row_query_with_an_odd_stride():
    from cclip_hip import ops
    g = rows16(5, seed=1)
    wide = torch.zeros(2, 37, dtype=torch.bfloat16, device="cuda")
    wide[:, :32] = rows16(2)
    s, i = ops.similarity_topk(wide[:1, :32], g, 2)
    s0, i0 = ops.similarity_topk(wide[:1, :32].contiguous(), g, 2)
    assert torch.equal(_bits(s), _bits(s0)) and torch.equal(i, i0)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.similarity_topk(wide[:, :32], g, 2)


def test_one_centroid_out_c_with_an_odd_stride():
    from cclip_hip import ops
    x, assign = rows16(3), torch.zeros(3, dtype=torch.int32, device="cuda")
    prev = rows16(2, seed=1)
    wide = torch.zeros(2, 37, dtype=torch.bfloat16, device="cuda")
    c, n, _ = ops.kmeans_update(x, assign, 1, prev[:1], out_c=wide[:1, :32])
    c0, n0, _ = ops.kmeans_update(x, assign, 1, prev[:1])
    assert c.data_ptr() == wide.data_ptr() and torch.equal(_bits(c), _bits(c0)) and torch.equal(_bits(n), _bits(n0))
    assert not wide[:, 32:].any() and not wide[1].any()
    short = torch.zeros(48, dtype=torch.bfloat16, device="cuda").as_strided((2, 32), (16, 1))       # rows that overlap
    with pytest.raises(ValueError, match="out_c"):
        ops.kmeans_update(x, torch.tensor([0, 1, 0], dtype=torch.int32, device="cuda"), 2, prev, out_c=short)
    torch.cuda.synchronize()
    assert not short.any()


def test_one_row_of_scores_with_a_short_stride():
    from cclip_hip import ops
    scores = torch.tensor([[0.9, 0.5, 0.1, 0.3, 0.2]] * 2, device="cuda")
    one = scores.as_strided((1, 5), (2, 1))                                     # a row stride below k: free for one row
    P, beta = ops.tsne_affinities(one, 2.0)
    P0, beta0 = ops.tsne_affinities(scores[:1].contiguous(), 2.0)
    assert torch.equal(_bits(P), _bits(P0)) and torch.equal(_bits(beta), _bits(beta0))
    P, beta = ops.tsne_affinities(torch.zeros(2, 7, device="cuda").copy_(torch.nn.functional.pad(scores, (0, 2)))[:1, :5], 2.0)   # an odd one
    assert torch.equal(_bits(P), _bits(P0)) and torch.equal(_bits(beta), _bits(beta0))
    with pytest.raises(ValueError, match="below k"):
        ops.tsne_affinities(scores.as_strided((2, 5), (2, 1)), 2.0)


def test_one_row_out_w_with_a_short_stride():
    """concept_codes rounds a one-row out_w's stride up to the 4 ceil(V / 4) it needs, not down to a multiple of 4: a short stride
    is taken, an odd one above V is refused as for two rows (the wrapper's behaviour since it was written, kept)"""
    from cclip_hip import ops
    x, c = rows16(1), rows16(6, seed=1)
    buf = f32(16)
    out = ops.concept_codes(x, c, 0.05, 0.5, 3, out_w=buf.as_strided((1, 6), (4, 1)))
    ref = ops.concept_codes(x, c, 0.05, 0.5, 3)
    assert out[0].data_ptr() == buf.data_ptr() and all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, ref))
    assert bool((buf[8:] == 7.0).all())
    for n_rows in (1, 2):
        wide = f32(2, 9)
        with pytest.raises(ValueError, match="multiple of 4"):
            ops.concept_codes(rows16(n_rows), c, 0.05, 0.5, 3, out_w=wide[:n_rows, :6])
        torch.cuda.synchronize()
        assert bool((wide == 7.0).all())
